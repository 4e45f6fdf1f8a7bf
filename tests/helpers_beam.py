"""Checking tools of the beam-search decode (decode.beam_decode, fn_beam_step / fn_beam_gather / fn_beam_backtrack): the definition of
include/fadernets.h restated in numpy fp32 on packed 64-bit words, a second plain-Python search written without them, numpy walks of the gather
and the backtrack, the checkers built on them, the fp64 replay of returned hypotheses and the FakeOps stand-in."""
import numpy as np
import torch

from fake_ops import FakeOps
from helpers import _DECODER_KEYS
from helpers_forced import replay_forced_check
from oracle import gmvae_oracle as orc

MAX_W = 16                                                     # FN_BEAM_MAX_W
# (B, W, V) of the fn_beam_step cases: three sequences' worth of wavefront rounds at the decoder's V, one beam, the widest beam (4 rows per wavefront),
# the 16-entries-per-lane instance at its ends (V = 385, 1024) with W not a multiple of the 4 wavefronts, two entries per lane (65), one entry in all
STEP_SHAPES = [(9, 4, 342), (1, 1, 342), (3, 16, 342), (5, 3, 1024), (2, 16, 385), (4, 2, 65), (2, 1, 1)]


def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a if dtype is None else np.ascontiguousarray(a, dtype=dtype)


def score_keys(s):
    """order-preserving uint32 key of fp32 scores: bits ^ (sign ? 0xffffffff : 0x80000000)"""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31) != 0, ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def key_scores(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k >> np.uint32(31) != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def reference_beam_step(lp_rows, W, step, eos=-1, score_prev=None, token_prev=None):
    """The definition on fp32 log-prob rows lp_rows (B*W, V): every candidate as the word pack(s, w*V + e), the W largest words per sequence.
    Returns (score (B, W) float32, parent (B, W) int32, token (B, W) int32)."""
    lp = _np(lp_rows, np.float32)
    R, V = lp.shape
    B = R // W
    assert B * W == R and 1 <= W <= min(V, MAX_W) and -1 <= eos < V
    lp = lp.reshape(B, W, V)
    n = W * V
    sp = np.zeros((B, W), dtype=np.float32) if step == 0 else _np(score_prev, np.float32).reshape(B, W)
    live = np.ones((B, W), bool) if step > 0 else np.broadcast_to(np.arange(W) == 0, (B, W))
    fin = np.zeros((B, W), bool) if step == 0 or eos < 0 else _np(token_prev).reshape(B, W) == eos
    with np.errstate(invalid="ignore", over="ignore"):
        s = (sp[:, :, None] + lp).astype(np.float32)                              # ONE fp32 add
    low = (n - 1 - np.arange(n, dtype=np.uint64)).reshape(1, W, V)
    words = (score_keys(s).astype(np.uint64) << np.uint64(32)) | low
    words = np.where((live & ~fin)[:, :, None], words, np.uint64(0))
    if fin.any():
        fw = (score_keys(sp).astype(np.uint64) << np.uint64(32)) | low[:, :, max(eos, 0)]
        words[:, :, max(eos, 0)] = np.where(fin, fw, words[:, :, max(eos, 0)])
    words = words.reshape(B, n)
    best = np.sort(words, axis=1)[:, ::-1][:, :W]                                 # the words are distinct (but for the empty ones): no ties left
    i =n - 1 - np.minimum(best & np.uint64(0xffffffff), np.uint64(n - 1)).astype(np.int64)
    return key_scores((best >> np.uint64(32)).astype(np.uint32)), (i // V).astype(np.int32), (i % V).astype(np.int32)


def python_beam_step(lp_rows, W, step, eos=-1, score_prev=None, token_prev=None):
    """The same step as a plain search over explicit hypothesis lists, written without the packed words: candidates (score, parent, token) sorted
    by (-score, parent, token).  (It orders -0.0 and +0.0 as equal where the word orders them; no input here has a score of either zero twice.)"""
    lp = _np(lp_rows, np.float32)
    R, V = lp.shape
    B = R // W
    out_s, out_p, out_t = [], [], []
    for b in range(B):
        hyps = []
        for w in range(W):
            if step == 0 and w > 0:
                continue
            sp = np.float32(0.0) if step == 0 else np.float32(_np(score_prev).reshape(B, W)[b, w])
            if step > 0 and eos >= 0 and int(_np(token_prev).reshape(B, W)[b, w]) == eos:
                hyps.append((sp, w, eos))
                continue
            for e in range(V):
                hyps.append((np.float32(sp + np.float32(lp[b * W + w, e])), w, e))
        hyps.sort(key=lambda h: (-float(h[0]), h[1], h[2]))
        out_s.append([h[0] for h in hyps[:W]]), out_p.append([h[1] for h in hyps[:W]]), out_t.append([h[2] for h in hyps[:W]])
    return np.array(out_s, dtype=np.float32), np.array(out_p, dtype=np.int32), np.array(out_t, dtype=np.int32)


def reference_gather(src, parent, W):
    """dst[r] = src[(r // W) * W + clamp(parent[r])]"""
    src, parent = _np(src), _np(parent).reshape(-1).astype(np.int64)
    r = np.arange(src.shape[0])
    return src[(r // W) * W + np.clip(parent, 0, W - 1)]


def reference_backtrack(parent, token, score, eos=-1):
    """numpy walk of the slabs [steps][B][W] -> dict(tokens, beam, cum (B, W, steps), lens, final (B, W))"""
    parent, token, score = _np(parent).astype(np.int64), _np(token), _np(score, np.float32)
    steps, B, W = parent.shape
    tokens, beam, cum = np.zeros((B, W, steps), np.int32), np.zeros((B, W, steps), np.int32), np.zeros((B, W, steps), np.float32)
    cur = np.broadcast_to(np.arange(W), (B, W)).copy()
    bb = np.arange(B)[:, None]
    for t in range(steps - 1, -1, -1):
        p = np.clip(parent[t][bb, cur], 0, W - 1)
        tokens[:, :, t], cum[:, :, t], beam[:, :, t] = token[t][bb, cur], score[t][bb, cur], p
        cur = p
    hit = tokens == eos if eos >= 0 else np.zeros_like(tokens, bool)
    lens = np.where(hit.any(2), hit.argmax(2) + 1, steps).astype(np.int32)
    return dict(tokens=tokens, beam=beam, cum=cum, lens=lens, final=score[steps - 1].copy())


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def beam_check_step(lp_rows, W, step, eos, score_prev, token_prev, score, parent, token):
    """one step's slabs against the restatement on the step's own log-prob rows and the previous slabs: scores bit for bit, parents and tokens exactly"""
    rs, rp, rt = reference_beam_step(lp_rows, W, step, eos, score_prev, token_prev)
    B = rs.shape[0]
    score, parent, token = _np(score, np.float32).reshape(B, W), _np(parent).reshape(B, W), _np(token).reshape(B, W)
    bad = (parent != rp) | (token != rt)
    if bad.any():
        b, j = (int(x) for x in np.argwhere(bad)[0])
        raise AssertionError("(sel) step %d sequence %d output %d: (parent, token) (%d, %d), definition (%d, %d); %d entries"
                             % (step, b, j, parent[b, j], token[b, j], rp[b, j], rt[b, j], int(bad.sum())))
    assert _same_bits(score, rs), "(score) step %d: scores differ from the definition's, max |d| %.3e" % (step, float(np.nanmax(np.abs(score - rs))))


def beam_check_gather(dst, src, parent, W):
    want, dst = reference_gather(src, parent, W), _np(dst)
    assert dst.shape == want.shape and np.array_equal(dst.view(np.uint32), want.view(np.uint32)), \
        "(gather) %d rows are not src[(r // W) * W + parent[r]]" % int((dst != want).any(1).sum())


def beam_check_backtrack(parent, token, score, eos, tokens, beam, cum, lens, final):
    ref = reference_backtrack(parent, token, score, eos)
    for name, got in (("tokens", tokens), ("beam", beam), ("lens", lens)):
        if got is not None:
            assert np.array_equal(_np(got), ref[name]), "(backtrack) %s differ from the walk at %d entries" % (name, int((_np(got) != ref[name]).sum()))
    for name, got in (("cum", cum), ("final", final)):
        if got is not None:
            assert _same_bits(_np(got), ref[name]), "(backtrack) %s differ from the walk" % name
    return ref


def beam_check_trace(trace, W, eos, tokens=None, scores=None, lens=None):
    """every step of a beam_decode(trace=True) against the restatement, then the backtrack; tokens / scores / lens: what beam_decode returned (checked
    through trace['order'])"""
    sc, pa, tk, rows = (_np(trace[k]) for k in ("score", "parent", "token", "rows"))
    steps = sc.shape[0]
    for i in range(steps):
        beam_check_step(rows[i], W, i, eos, sc[i - 1] if i else None, tk[i - 1] if i else None, sc[i], pa[i], tk[i])
    ref = beam_check_backtrack(pa, tk, sc, eos, None, trace["beam"], trace["cum"], None, None)
    order = _np(trace["order"])
    bb = np.arange(order.shape[0])[:, None]
    for name, got in (("tokens", tokens), ("lens", lens)):
        if got is not None:
            assert np.array_equal(_np(got), ref[name][bb, order]), "(backtrack) returned %s differ from the walk" % name
    if scores is not None:
        assert _same_bits(_np(scores), ref["final"][bb, order]), "(backtrack) returned scores differ from the last slab"
    return ref


def beam_replay_check(sd, z, tokens_j, scores_j, logp_j, rows, lens_j=None):
    """Hypothesis j of every sequence in `rows` (tokens_j (Bi, steps), scores_j (Bi,), logp_j (Bi, steps, 342) = the model's own log-probs gathered along
    its path) against an fp64 replay with every step forced to its own tokens: the rules, tolerance and cap of helpers_forced.replay_forced_check, and
    |score - sum_i lp64[tok_i]| <= steps * tol_lp + steps * 2^-24 * |score| (each of the steps adds a log-prob within tol_lp of the fp64 one and rounds
    the sum once; a hypothesis that ended sums the positions before its end).  Returns replay_forced_check's figures + max_dscore."""
    tokens_j = torch.as_tensor(tokens_j).detach().cpu().long()
    Bi, steps = tokens_j.shape
    lg = torch.as_tensor(logp_j).detach().cpu()
    own = torch.from_numpy(np.argmax(lg.numpy(), axis=-1))
    st = replay_forced_check(sd, z, own, tokens_j, np.ones(steps, dtype=bool), tokens_j, lg, rows=rows)
    rows = torch.as_tensor(rows, dtype=torch.long)
    dec = {k: v.detach().cpu().double() for k, v in sd.items() if k.startswith(_DECODER_KEYS)}
    with torch.no_grad():
        lp64 = orc.global_decoder(dec, torch.as_tensor(z).detach().cpu()[rows].double(), steps, teacher=tokens_j[rows])
    along = lp64.gather(-1, tokens_j[rows].unsqueeze(-1)).squeeze(-1)
    if lens_j is not None:
        along = along * (torch.arange(steps).view(1, -1) < torch.as_tensor(lens_j).detach().cpu().long()[rows].view(-1, 1))
    sc = torch.as_tensor(scores_j).detach().cpu().double()[rows]
    err = (sc - along.sum(1)).abs()
    bound = steps * st["tol_lp"] + steps * 2.0 ** -24 * sc.abs()
    st["max_dscore"] = float(err.max())
    bad = ~(err <= bound)
    assert not bool(bad.any()), "(sum) |score - sum lp64[tok]| = %.3e above %.3e at row %d, %d rows" % (
        float(err[bad].max()), float(bound[bad].min()), int(rows[torch.nonzero(bad)[0, 0]]), int(bad.sum()))
    return st


def beam_line(tag, W, st):
    return "%-34s W %2d Bi %4d steps %3d rows %3d  e_ref %.3e  max|dlogp| %.3e  max|dscore| %.3e  below_delta %.3f %%" % (
        tag, W, st["Bi"], st["steps"], st["rows"], st["e_ref"], st["max_dlp"], st["max_dscore"], 100 * st["share_below_delta"])


def step_inputs(B, W, V, step, eos, seed, ld=None):
    """logits (B*W, ld) with padding that is no logit, score_prev, token_prev for one fn_beam_step case, with planted trouble: sequence 0 has identical
    beam rows and equal previous scores (ties between beams), row 0 of every sequence two pairs of equal logits at its top (ties inside a row);
    step 0: NaN rows for the beams w > 0; eos >= 0 at step > 0: every other beam finished, its row NaN"""
    g = torch.Generator().manual_seed(seed)
    ld = ld or V
    x = torch.full((B * W, ld), 1e9)
    x[:, :V] = torch.randn(B * W, V, generator=g) * 4
    xs = x.view(B, W, ld)
    if V >= 4:
        top = xs[:, 0, :V].max(1)[0] + 1
        xs[:, 0, V - 1], xs[:, 0, 1] = top, top
        xs[:, 0, 2], xs[:, 0, 0] = top - 0.5, top - 0.5
    xs[0, :, :V] = xs[0, 0, :V].clone()
    sp = -torch.rand(B, W, generator=g) * 30
    sp[0] = sp[0, 0]
    if B > 1 and W > 1:
        sp[1, 1] = sp[1, 0]
    tp = torch.randint(0, V, (B, W), generator=g, dtype=torch.int32)
    if eos >= 0:
        tp[tp == eos] = (eos + 1) % V
    if step == 0:
        xs[:, 1:, :V] = float("nan")
    elif eos >= 0:
        tp[:, 1::2] = eos
        xs[:, 1::2, :V] = float("nan")
    return x, sp, tp


class BeamFakeOps(FakeOps):
    """FakeOps + the three beam entry points as their numpy restatements"""

    def beam_step(self, logits, W, V, step, eos, score_prev, token_prev, score, parent, token, logp_out=None):
        self.calls.append("beam_step")
        lp = torch.log_softmax(logits[:, :V], dim=-1)
        s, p, t = reference_beam_step(lp.numpy(), W, step, eos, score_prev, token_prev)
        score.copy_(torch.from_numpy(s)), parent.copy_(torch.from_numpy(p)), token.copy_(torch.from_numpy(t))
        if logp_out is not None:
            logp_out.copy_(lp)

    def beam_gather(self, jobs, parent, W):
        self.calls.append("beam_gather")
        for src, dst in jobs:
            assert src.data_ptr() != dst.data_ptr()
            dst.copy_(torch.from_numpy(reference_gather(src, parent, W)))

    def beam_backtrack(self, parent, token, score, eos, tokens_out, len_out, score_out, beam_out=None, cum_out=None):
        self.calls.append("beam_backtrack")
        ref = reference_backtrack(parent, token, score, eos)
        for out, k in ((tokens_out, "tokens"), (len_out, "lens"), (score_out, "final"), (beam_out, "beam"), (cum_out, "cum")):
            if out is not None:
                out.copy_(torch.from_numpy(ref[k]))


# the end-to-end cases of tests/test_gpu_beam.py, (weights, Bi, W, steps, arith); z = helpers.replay_z(Bi, Z, Bi).  tests/test_beam.py runs the replayed
# rows of each through the stand-in, which shows that these inputs stay under helpers.REPLAY_CAP on the reference alone
BEAM_CASES = [("h64", 5, 4, 24, None), ("h512", 177, 4, 16, None), ("h512", 256, 8, 12, "bf16x6")]
BEAM_REPLAY_ROWS = 32


def beam_rows(Bi):
    from helpers import replay_rows
    return replay_rows(Bi, n=BEAM_REPLAY_ROWS)
