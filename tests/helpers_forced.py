"""Checking tools of the forced-feedback decode (greedy_decode(..., forced, force), fn_decode_forced, continue_from, scheduled sampling),
next to helpers.replay_decode_check, whose rules, tolerance and cap they apply to a decode that was fed a GIVEN stream."""
import os
import time

import numpy as np
import torch

from helpers import _DECODER_KEYS, NOISE_PARAMS, REPLAY_CAP, replay_rows
from oracle import gmvae_oracle as orc

FORCED_MASKS = ("prefix", "bernoulli", "all")
# the decode cases tests/test_gpu_forced.py forces, (path, weights, Bi, steps); paths as in helpers.REPLAY_CASES: the one-launch kernel as one
# block (1, 17, 32 rows), as its 32-row pipeline (33, 352 rows) and its 64-row pipeline (353, 2048 rows); the per-token scan steps, fp32
# cells and bf16 x 6 cells (2048 rows), whose cached graphs also replay a second forced batch and a second mask (seed Bi + 1)
FORCED_CASES = [
    ("one_launch", "h64", 1, 300), ("one_launch", "h512", 17, 300), ("one_launch", "h512", 32, 300),
    ("pipeline32", "h512", 33, 250), ("pipeline32", "h64", 352, 200),
    ("pipeline64", "h512", 353, 150), ("pipeline64", "h64", 2048, 120),
    ("scan_steps", "h64", 17, 200), ("cells_f32", "h512", 705, 100), ("cells_x6", "h512", 2048, 100),
]
FORCED_GRAPH_PATHS = ("scan_steps", "cells_f32", "cells_x6")


def forced_mask(kind, steps, seed=0):
    """the three mask shapes of the forced-decode tests: a prefix of P = steps // 3, a seeded Bernoulli(0.5), every step forced"""
    if kind == "prefix":
        return np.arange(steps) < max(1, steps // 3)
    if kind == "bernoulli":
        return np.random.RandomState(1000 + seed).rand(steps) < 0.5
    if kind == "all":
        return np.ones(steps, dtype=bool)
    if kind == "none":
        return np.zeros(steps, dtype=bool)
    raise ValueError(kind)


def forced_tokens(Bi, steps, seed, V=orc.E):
    """random tokens to force, from their own generator"""
    return torch.randint(0, V, (Bi, steps), generator=torch.Generator().manual_seed(77 + seed), dtype=torch.int64)


def fed_stream(tokens, forced, force):
    """fed[b][i] = force[i] ? forced[b][i] : tokens[b][i]"""
    tokens = torch.as_tensor(tokens).detach().cpu().long()
    m = torch.as_tensor(np.asarray(force, dtype=bool)).view(1, -1)
    return torch.where(m, torch.as_tensor(forced).detach().cpu().long()[:, :tokens.shape[1]], tokens)


def oracle_forced_decode(sd, z, steps, forced, force):
    """gmm_model.py:119-149 with a per-step choice of the feedback (:139-148): forced[:, i] where force[i], else the first-index argmax.
    Plain torch in the dtype of sd / z -> (log-probs (B, steps, E), own argmax tokens (B, steps)).  With force all True this IS
    orc.global_decoder(teacher=forced), with force all False orc.greedy_decode."""
    B = z.shape[0]
    forced = torch.as_tensor(forced).long()
    tok = torch.full((B,), orc.START_TOKEN, dtype=torch.long)
    hx0 = z @ sd["linear_init_global.weight"].t() + sd["linear_init_global.bias"]
    hx1 = None
    outs = []
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
            tok = forced[:, i] if force[i] else out.max(1)[1]
    lp = torch.stack(outs, dim=1)
    return lp, lp.argmax(-1)


def replay_forced_check(sd, z, tokens, forced, force, fed, logp=None, rows=None):
    """Every step of a forced-feedback decode against an fp64 replay of the stream it was FED.

    tokens / logp are the decoder's OWN first-index argmax and log-probs of every step; fed is the stream the path under test reports
    as fed back.  First fed == where(force, forced, tokens) is asserted exactly (force[steps-1] plays no part in the decode, but the
    identity holds there as well).  Then the oracle decoder replays teacher=fed in fp64 and fp32, and the rules of
    helpers.replay_decode_check hold for the own tokens and log-probs with the same tolerance tol_lp = min(1e-4, 16 e_ref),
    delta = 2 tol_lp and the same cap REPLAY_CAP on the share of positions whose fp64 top-2 gap is below delta:
      (a) |lp - lp64| <= tol_lp over all 342 entries;   (b) the token is the first-index argmax of the own log-prob row;
      (c) lp64[tok] >= max(lp64) - delta.
    A decode that fed its argmax at a forced step (or the forced token at a free one) computed later steps from another stream
    than fed: (a) / (c) fail there.  Returns the figures as a dict."""
    t0 = time.time()
    tokens = torch.as_tensor(tokens).detach().cpu().long()
    fed = torch.as_tensor(fed).detach().cpu().long()
    forced = torch.as_tensor(forced).detach().cpu().long()
    force = np.asarray(force, dtype=bool)
    Bi, steps = tokens.shape
    assert force.shape == (steps,) and tuple(fed.shape) == (Bi, steps) and forced.shape[0] == Bi and forced.shape[1] >= steps
    want = fed_stream(tokens, forced, force)
    bad = fed != want
    if bool(bad.any()):
        r, s = (int(x) for x in torch.nonzero(bad)[0])
        raise AssertionError("(fed) fed != where(force, forced, tokens) at row %d step %d (force %d): fed %d, forced %d, own %d; %d positions"
                             % (r, s, int(force[s]), int(fed[r, s]), int(forced[r, s]), int(tokens[r, s]), int(bad.sum())))
    rows = torch.as_tensor(replay_rows(Bi) if rows is None else rows, dtype=torch.long)
    tk, fd = tokens[rows], fed[rows]
    E = orc.E
    assert int(tk.min()) >= 0 and int(tk.max()) < E and int(fd.min()) >= 0 and int(fd.max()) < E, "token out of range"
    zr = torch.as_tensor(z).detach().cpu()[rows]
    dec = {k: v.detach().cpu() for k, v in sd.items() if k.startswith(_DECODER_KEYS)}
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    try:
        with torch.no_grad():
            lp64 = orc.global_decoder({k: v.double() for k, v in dec.items()}, zr.double(), steps, teacher=fd)
            lp32 = orc.global_decoder({k: v.float() for k, v in dec.items()}, zr.float(), steps, teacher=fd)
    finally:
        torch.set_num_threads(threads)
    assert lp64.dtype == torch.float64 and lp32.dtype == torch.float32
    e_ref = float((lp32.double() - lp64).abs().max())
    tol = min(1e-4, 16.0 * e_ref)
    delta = 2.0 * tol
    top2 = lp64.topk(2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]
    share = float((gap < delta).double().mean())
    st = dict(Bi=Bi, steps=steps, rows=len(rows), positions=tk.numel(), e_ref=e_ref, tol_lp=tol, delta=delta, share_below_delta=share,
              max_dlp=float("nan"), ratio=float("nan"), forced_share=float(force[:steps - 1].mean()) if steps > 1 else 0.0)

    def where(mask):
        r, s = (int(x) for x in torch.nonzero(mask)[0])
        return "row %d step %d" % (int(rows[r]), s)

    if logp is not None:
        lg = torch.as_tensor(logp).detach().cpu()[rows].double()
        assert tuple(lg.shape) == (len(rows), steps, E), tuple(lg.shape)
        err = (lg - lp64).abs().amax(-1)                                   # NaN stays NaN: fails the bound below
        st["max_dlp"] = float(err.max())
        st["ratio"] = st["max_dlp"] / max(e_ref, 1e-30)
        bad = ~(err <= tol)
        assert not bool(bad.any()), "(a) |lp_gpu - lp64| = %.3e > tol_lp %.3e (e_ref %.3e) at %s, %d positions" % (
            float(err[bad].max()), tol, e_ref, where(bad), int(bad.sum()))
        own = torch.from_numpy(np.argmax(lg.numpy(), axis=-1))             # numpy: first index of the maximum
        bad = own != tk
        assert not bool(bad.any()), "(b) token is not the first-index argmax of the kernel's own log-probs at %s, %d positions" % (
            where(bad), int(bad.sum()))
    short = top2[..., 0] - lp64.gather(-1, tk.unsqueeze(-1)).squeeze(-1)
    bad = short > delta
    assert not bool(bad.any()), "(c) lp64[tok] is %.3e below the fp64 best (delta %.3e) at %s, %d positions" % (
        float(short[bad].max()), delta, where(bad), int(bad.sum()))
    assert share <= REPLAY_CAP, "cap: %.2f %% of the positions have an fp64 top-2 gap below delta %.3e" % (100 * share, delta)
    st["seconds"] = time.time() - t0
    return st


def forced_line(path, mask, H, st):
    return ("%-22s %-9s Bi %4d H %3d steps %3d rows %3d  forced %.2f  e_ref %.3e  max|dlogp| %.3e  ratio %6.3f  below_delta %.3f %%  replay %.1f s"
            % (path, mask, st["Bi"], H, st["steps"], st["rows"], st["forced_share"], st["e_ref"], st["max_dlp"], st["ratio"],
               100 * st["share_below_delta"], st["seconds"]))


# ------------------------------------------------------------------------------------------------------------------------------
# scheduled sampling in the drop-in classes (model.eps < 1, gmm_model.py:139-144)
# ------------------------------------------------------------------------------------------------------------------------------
def check_scheduled_sampling(pkg, m, batch, dev, seed=31, eps=0.5, tol_grad=3e-4):
    """One train-mode model(...) call with model.eps = eps under a seeded generator, then a reference-style loss and loss.backward():
      - the mask is `rand(1) < eps` over the T draws the reference makes after its two randn(B, Z) draws (same generator order);
      - fed == where(mask, x, pass-1 tokens) exactly, and `out` - the log-probs of pass 2 - passes replay_forced_check with teacher = fed
        (the pass-1 tokens must be out's own first-index argmax, its log-probs within tol_lp of the fp64 replay);
      - every parameter gradient matches autograd through the fp64 oracle run with teacher = fed (relative to the tensor's max: tol_grad,
        the tolerance of test_host_logic.test_dropin_forward_and_autograd).
    batch: synth_batch dict.  Returns the replay figures."""
    from helpers import relerr
    d, r, n = (torch.from_numpy(batch[k]).long() for k in ("d", "r", "n"))
    c = torch.from_numpy(batch["c"]).float()
    B, T = d.shape
    Z = m.latent_dim
    sd32 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    m.train()
    m.eps = eps
    m.zero_grad()
    torch.manual_seed(seed)
    er, en = torch.randn(B, Z), torch.randn(B, Z)
    draws = [float(torch.rand(1)) for _ in range(T)]
    mask = np.array([p < eps for p in draws])
    assert 0 < mask[:T - 1].sum() < T - 1
    after_ref = float(torch.rand(1))               # where the reference's draws leave the generator
    torch.manual_seed(seed)
    res = m(pkg.convert_to_one_hot(d.to(dev), 342), pkg.convert_to_one_hot(r.to(dev), 3), pkg.convert_to_one_hot(n.to(dev), 16), c.to(dev))
    assert float(torch.rand(1)) == after_ref, "the call consumed the generator differently from the reference"
    (out, r_out, n_out, _, _), (dis_r, dis_n), (z_r, z_n), (ll_r, ll_n), (qy_r, qy_n), _ = res
    assert m._ss == tuple(bool(x) for x in mask), "the mask is not `rand(1) < eps` over the reference's draws"
    fed, own = m.fed.cpu().long(), m.sampled.cpu().long()
    zc = torch.cat([z_r, z_n, c.to(dev)], dim=1).detach().cpu()
    st = replay_forced_check(sd32, zc, own, d, mask, fed, out.detach().cpu())
    # reference-style loss on OUR outputs, as trainer_gmm.py would compute it
    got = dict(out=out, r_out=r_out, n_out=n_out, mu_r=dis_r.mean, sigma_r=dis_r.stddev, mu_n=dis_n.mean, sigma_n=dis_n.stddev,
               z_r=z_r, z_n=z_n, ll_r=ll_r, ll_n=ll_n, qy_r=qy_r, qy_n=qy_n)
    got = {k: v.cpu() for k, v in got.items()}              # the oracle's loss is CPU torch; .cpu() passes the gradients back
    params = {k: p.cpu() for k, p in m.named_parameters()}
    ls = orc.loss_function(params, got, d, r, n, 20000, beta=0.2)
    l_r, l_n = orc.latent_regularized_loss(got["z_r"], got["z_n"], batch["r_density"], batch["n_density"])
    (ls[0] + l_r + l_n).backward()
    # fp64 oracle with teacher = fed, autograd
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    try:
        sd = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in sd32.items()}
        fw = orc.forward(sd, d, r, n, c.double(), er.double(), en.double(), training=True)
        fw["out"] = orc.global_decoder(sd, torch.cat([fw["z_r"], fw["z_n"], c.double()], dim=1), T, teacher=fed)
        ls64 = orc.loss_function(sd, fw, d, r, n, 20000, beta=0.2)
        l_r64, l_n64 = orc.latent_regularized_loss(fw["z_r"], fw["z_n"], batch["r_density"], batch["n_density"])
        loss64 = ls64[0] + l_r64 + l_n64
        keys = [k for k, v in sd.items() if v.requires_grad]
        grads = dict(zip(keys, torch.autograd.grad(loss64, [sd[k] for k in keys], allow_unused=True)))
    finally:
        torch.set_default_dtype(old)
        torch.set_num_threads(threads)
    assert abs(float((ls[0] + l_r + l_n).detach()) - float(loss64.detach())) <= 1e-4 * abs(float(loss64))
    checked = 0
    for k, p in m.named_parameters():
        ref = grads.get(k)
        if "lookup" in k or k in NOISE_PARAMS:        # mixture lookups: not encoder / decoder parameters; zero-gradient biases (helpers.NOISE_PARAMS)
            continue
        if ref is None or p.grad is None:
            assert ref is None or float(ref.abs().max()) < 1e-6, k
            continue
        ref = ref.numpy()
        e = relerr(p.grad.cpu().numpy(), ref)
        assert e < tol_grad or np.abs(ref).max() < 1e-6, (k, e)
        checked += 1
    assert checked >= 20
    st["grads_checked"] = checked
    return st
