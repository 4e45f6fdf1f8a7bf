"""Checking tools of the seeded sampling decode (decode.sample_decode, fn_vocab_sample): Philox4x32-10 and the uniforms in numpy, the
definition of include/fadernets.h restated in fp64 / fp32, the checker of drawn tokens, an oracle decode loop and the FakeOps stand-in."""
import numpy as np
import torch

from fake_ops import FakeOps
from helpers import REPLAY_CAP
from oracle import gmvae_oracle as orc

SETTINGS = [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 8, 1.0), (1.0, 0, 0.9), (0.8, 40, 0.95)]      # (temperature, top_k, top_p)
PARAMS_DTYPE = [("seed", "<u8"), ("offset", "<u8"), ("inv_t", "<f4"), ("top_p", "<f4"), ("top_k", "<i4"), ("reserved", "<i4")]      # FnSampleParams
MIN_P, MIN_INV_T, MAX_INV_T = np.float32(1e-30), np.float32(1e-30), np.float32(1e30)          # FN_SAMPLE_* of include/fadernets.h


def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) uint32 -> (..., 4) uint32 (Salmon et al. 2011, ten rounds)"""
    c = np.array(np.broadcast_arrays(*[np.asarray(counter, dtype=np.uint64)[..., i] for i in range(4)]))
    k0, k1 = (np.asarray(key, dtype=np.uint64)[..., i] for i in range(2))
    c0, c1, c2, c3 = c
    M = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def sample_uniforms(rows, steps, seed=0, offset=0):
    """u[r][s] of batch rows `rows` at steps `steps`: (Philox(counter = (row, step, offset_lo, offset_hi), key = (seed_lo, seed_hi))[0] >> 8) * 2^-24,
    float32, exact"""
    rows, steps = np.asarray(rows, dtype=np.uint64).reshape(-1, 1), np.asarray(steps, dtype=np.uint64).reshape(1, -1)
    ctr = np.stack(np.broadcast_arrays(rows, steps, np.uint64(offset & 0xffffffff), np.uint64(offset >> 32)), axis=-1)
    out = philox4x32_10(ctr, np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64))
    return ((out[..., 0] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def clamp_settings(T=None, k=0, p=1.0, V=orc.E, inv_t=None):
    """(inv_temperature fp32, top_k, top_p fp32) as the kernel and its host twin clamp what they read from memory"""
    with np.errstate(over="ignore", divide="ignore"):
        it = np.float32(inv_t) if inv_t is not None else np.float32(1.0) / np.float32(T)
    it = np.float32(1.0) if np.isnan(it) else np.float32(min(max(it, MIN_INV_T), MAX_INV_T))
    p = np.float32(p)
    p = np.float32(1.0) if not p <= 1 else np.float32(max(p, MIN_P))
    return it, int(min(max(int(k), 0), V)), p


def _prefix_sums(w):
    """inclusive prefix sums of w (N, V) in w's dtype and in the order include/fadernets.h sets: 64 blocks of per = ceil(V / 64) entries summed in
    order, the block totals scanned (t[l] += t[l - o] for o = 1, 2, .. 32), c = total of the blocks before + the running sum inside the block"""
    N, V = w.shape
    per = -(-V // 64)
    wp = np.zeros((N, 64 * per), dtype=w.dtype)
    wp[:, :V] = w
    run = np.cumsum(wp.reshape(N, 64, per), axis=2, dtype=w.dtype)
    tot = run[:, :, -1].copy()
    o = 1
    while o < 64:
        tot[:, o:] = tot[:, o:] + tot[:, :-o]
        o *= 2
    before = np.concatenate([np.zeros((N, 1), dtype=w.dtype), tot[:, :-1]], axis=1)
    return (before[:, :, None] + run).reshape(N, 64 * per)[:, :V]


def sample_rows(lp32, u, T, k, p, dtype=np.float64, inv_t=None):
    """The definition, for N rows at once, on fp32 log-prob rows lp32 (N, V) and uniforms u (N,), in `dtype` arithmetic, the prefix sums in the definition's order.
    The order (descending lp, ties to the lower index) and so the top-k set are exact in either dtype.  Returns a dict: tok (N,), order (N, V),
    n, m (N,), mass (N, V) = c / c[n-1], cdf (N, V) = c / c[m-1]."""
    lp32 = np.ascontiguousarray(lp32, dtype=np.float32)
    N, V = lp32.shape
    it, k, p = clamp_settings(T, k, p, V, inv_t)
    order = np.argsort(-lp32, axis=1, kind="stable")
    lps = np.take_along_axis(lp32, order, axis=1).astype(dtype)
    w = np.exp((lps - lps[:, :1]) * dtype(it))
    c = _prefix_sums(w)
    n = k if k else V
    ar = np.arange(N)
    m = np.full(N, n)
    if p < 1:
        thr = dtype(p) * c[:, n - 1]
        m = np.minimum(1 + (c[:, :n] < thr[:, None]).sum(1), n)
    cm = c[ar, m - 1]
    t = np.asarray(u, dtype=np.float32).astype(dtype) * cm
    j = np.minimum(((c <= t[:, None]) & (np.arange(V)[None, :] < m[:, None])).sum(1), m - 1)
    return dict(tok=order[ar, j], order=order, n=n, m=m, mass=c / c[:, n - 1:n], cdf=c / cm[:, None])


def reference_sample(lp32_row, u, T, k, p, dtype=np.float64):
    """one row: the drawn token"""
    return int(sample_rows(np.asarray(lp32_row)[None, :], np.asarray([u]), T, k, p, dtype)["tok"][0])


def sample_check(logp, tokens, u, params):
    """Drawn tokens against the fp64 definition evaluated on the kernel's OWN fp32 log-prob rows (so the order and the top-k set are exact).

    logp (N, V) float32, tokens (N,), u (N,) float32; params: dict(T, k, p).  e_cdf = max |cdf32 - cdf64| over the checked positions (prefix
    masses c / c[n-1] and draw boundaries c / c[m-1]) is what fp32 summation alone costs; delta = min(1e-4, 16 e_cdf).  A position is NEAR if u
    is within delta of an fp64 boundary between two kept tokens, or a prefix mass is within delta of top_p.  Off the near positions the token
    equals the fp64 token; at near ones it lies in the fp64 kept set plus the next-ranked token; at most REPLAY_CAP of the positions are
    near (a condition on the inputs).  Returns the figures and the near mask."""
    logp = np.asarray(torch.as_tensor(logp).detach().cpu().numpy() if torch.is_tensor(logp) else logp, dtype=np.float32)
    tokens = np.asarray(torch.as_tensor(tokens).detach().cpu().numpy() if torch.is_tensor(tokens) else tokens).astype(np.int64).reshape(-1)
    u = np.asarray(torch.as_tensor(u).detach().cpu().numpy() if torch.is_tensor(u) else u, dtype=np.float32).reshape(-1)
    N, V = logp.shape
    assert tokens.shape == (N,) and u.shape == (N,)
    assert np.isfinite(logp).all(), "log-probs not finite"
    assert tokens.min() >= 0 and tokens.max() < V, "token out of range"
    T, k, p = params["T"], params["k"], params["p"]
    r64 = sample_rows(logp, u, T, k, p, np.float64)
    r32 = sample_rows(logp, u, T, k, p, np.float32)
    n, m64 = r64["n"], r64["m"]
    col = np.arange(V)[None, :]
    mm = np.where(m64 == r32["m"], m64, 0)[:, None]          # the boundaries c / c[m-1] compare where both dtypes keep the same prefix
    e_cdf = max(float(np.abs(r32["mass"][:, :n].astype(np.float64) - r64["mass"][:, :n]).max()),
                float(np.where(col < mm, np.abs(r32["cdf"].astype(np.float64) - r64["cdf"]), 0.0).max()))
    delta = min(1e-4, 16.0 * e_cdf)
    near = ((np.abs(u.astype(np.float64)[:, None] - r64["cdf"]) <= delta) & (col < m64[:, None] - 1)).any(1)
    _, _, pc = clamp_settings(T, k, p, V)
    if pc < 1:
        near |= (np.abs(r64["mass"][:, :n] - float(pc)) <= delta).any(1)
    share = float(near.mean())
    st = dict(positions=N, e_cdf=e_cdf, delta=delta, near=near, share_near=share, tok64=r64["tok"], m64=m64)
    bad = ~near & (tokens != r64["tok"])
    assert not bad.any(), "(tok) token %d is not the fp64 draw %d at position %d (u %.8f, delta %.3e), %d positions" % (
        tokens[bad][0], r64["tok"][bad][0], np.nonzero(bad)[0][0], u[bad][0], delta, int(bad.sum()))
    rank = np.empty_like(r64["order"])
    np.put_along_axis(rank, r64["order"], np.broadcast_to(col, (N, V)), axis=1)
    bad = near & (rank[np.arange(N), tokens] > m64)
    assert not bad.any(), "(set) token outside the fp64 kept set + 1 at near position %d, %d positions" % (np.nonzero(bad)[0][0], int(bad.sum()))
    assert share <= REPLAY_CAP, "cap: %.2f %% of the positions are near a boundary (delta %.3e)" % (100 * share, delta)
    return st


def sample_check_decode(logp, tokens, rows, params, P=0):
    """every drawn position (steps >= P: the prompt's positions are no draws) of rows `rows` of a decode: logp (R, steps, V), tokens (R, steps)
    already restricted to those rows; params: dict(T, k, p, seed, offset)"""
    logp = torch.as_tensor(logp).detach().cpu().numpy()
    tokens = torch.as_tensor(tokens).detach().cpu().numpy()
    R, steps, V = logp.shape
    u = sample_uniforms(rows, np.arange(steps), params.get("seed", 0), params.get("offset", 0))
    st = sample_check(logp[:, P:].reshape(-1, V), tokens[:, P:].reshape(-1), u[:, P:].reshape(-1), params)
    st["near"] = np.concatenate([np.zeros((R, P), bool), st["near"].reshape(R, steps - P)], axis=1)
    return st


def sample_line(tag, params, st):
    return "%-30s T %.2f k %3d p %.2f  positions %6d  e_cdf %.3e  delta %.3e  near %.3f %%" % (
        tag, params["T"], params["k"], params["p"], st["positions"], st["e_cdf"], st["delta"], 100 * st["share_near"])


def oracle_sample_decode(sd, z, steps, T=1.0, k=0, p=1.0, seed=0, offset=0, prompt=None, dtype=np.float32):
    """gmm_model.py:119-149 with the draw of include/fadernets.h in place of _sampling, plain torch in the dtype of sd / z; the draw itself on
    the fp32 log-prob row in `dtype` -> (log-probs (B, steps, E), fed tokens (B, steps): the draws, the prompt in its first P columns)"""
    B = z.shape[0]
    P = 0 if prompt is None else prompt.shape[1]
    tok = torch.full((B,), orc.START_TOKEN, dtype=torch.long)
    hx0 = z @ sd["linear_init_global.weight"].t() + sd["linear_init_global.bias"]
    hx1 = None
    outs, toks = [], []
    u = sample_uniforms(np.arange(B), np.arange(steps), seed, offset)
    with torch.no_grad():
        for i in range(steps):
            inp = torch.cat([orc.convert_to_one_hot(tok, orc.E).to(z.dtype), z], dim=1)
            xp = inp @ sd["grucell_g.weight_ih"].t() + sd["grucell_g.bias_ih"]
            hx0 = orc.gru_cell(xp, hx0, sd["grucell_g.weight_hh"], sd["grucell_g.bias_hh"])
            if i == 0:
                hx1 = hx0
            xp2 = hx0 @ sd["grucell_g_2.weight_ih"].t() + sd["grucell_g_2.bias_ih"]
            hx1 = orc.gru_cell(xp2, hx1, sd["grucell_g_2.weight_hh"], sd["grucell_g_2.bias_hh"])
            out = torch.log_softmax(hx1 @ sd["linear_out_g.weight"].t() + sd["linear_out_g.bias"], dim=1)
            outs.append(out)
            if i < P:
                tok = torch.as_tensor(prompt)[:, i].long()
            else:
                tok = torch.from_numpy(sample_rows(out.float().numpy(), u[:, i], T, k, p, dtype)["tok"]).long()
            toks.append(tok)
    return torch.stack(outs, dim=1), torch.stack(toks, dim=1)


class SamplingFakeOps(FakeOps):
    """FakeOps + fn_vocab_sample as an fp32 numpy restatement of its definition"""

    def vocab_sample(self, logits, E, params, step, logp_out, tok_out, own_out=None, u_out=None):
        self.calls.append("vocab_sample")
        raw = params.cpu().numpy().view(PARAMS_DTYPE)[0]
        lp = torch.log_softmax(logits[:, :E], dim=-1)
        u = sample_uniforms(np.arange(logits.shape[0]), [step], int(raw["seed"]), int(raw["offset"]))[:, 0]
        r = sample_rows(lp.numpy(), u, None, int(raw["top_k"]), raw["top_p"], np.float32, inv_t=raw["inv_t"])
        if logp_out is not None:
            logp_out.copy_(lp)
        tok_out.copy_(torch.from_numpy(r["tok"]).to(torch.int32))
        if own_out is not None:
            own_out.copy_(logits[:, :E].max(1)[1].to(torch.int32))
        if u_out is not None:
            u_out.copy_(torch.from_numpy(u))
