"""Shared helpers for the parity tests: golden loading, model construction, comparisons."""
import os
import time

import numpy as np
import torch

from mfn_import import load_package
from oracle import gmvae_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOISE_PARAMS = ("linear_out_r.bias", "linear_out_n.bias")     # zero-gradient parameters, see test_oracle_golden.py


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def sd_from(g, pfx):
    return {k[len(pfx):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pfx)}


def batch_of(g):
    return {k: g[k] for k in ("d", "r", "n", "c", "r_density", "n_density", "a")}


def make_model(hidden, zdim, sd=None, device="cpu", ops=None, seed=1234, arith=None):
    pkg = load_package()
    torch.manual_seed(seed)
    m = pkg.MusicAttrRegGMVAE(roll_dims=342, rhythm_dims=3, note_dims=16, chroma_dims=24, hidden_dims=hidden, z_dims=zdim,
                              n_step=32, n_component=2)
    if sd is not None:
        m.load_state_dict(sd)
    m = m.to(device)
    if ops is not None:
        m._make_ops = lambda dev, _ops=ops: _ops          # test-side injection of the CPU stand-in for the kernel table
    m.train()
    if arith is not None:
        m.set_arith(arith)                                # "f32" / "bf16x6": arithmetic of the deep MFMA products (arith.py)
    return m


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def oracle_grads_f64(gold, sd32, sup=False):
    """Gradients of the training loss evaluated by the oracle in float64 ("exact" arithmetic).

    The q(y|x) softmax of gmm_model.py:217 takes log-likelihoods of magnitude ~1e3 whose float32 ulp is ~1e-4; when the
    posterior is not saturated every float32 implementation - the reference included - carries ~1e-3 relative noise in
    the gradients that flow through it.  Parity for those tensors is therefore stated as "no further from the float64
    truth than the reference itself (x4), or 5e-4"."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        sd = {k: v.double() for k, v in sd32.items()}
        grads, tup, _ = orc.gradients(sd, batch_of(gold), torch.from_numpy(gold["eps_r"]).double(),
                                      torch.from_numpy(gold["eps_n"]).double(), 20000, 0.2, is_supervised=sup)
    finally:
        torch.set_default_dtype(old)
    return {k: v.numpy() for k, v in grads.items()}


def grad_tolerances(gold, tag, exact):
    """per-parameter tolerance = max(5e-4, 4 x the reference's own distance from the float64 result)."""
    tol = {}
    for k, ex in exact.items():
        ref = gold["grad_%s/%s" % (tag, k)]
        tol[k] = max(5e-4, 4.0 * relerr(ref, ex))
    return tol


def epoch_loaders(g):
    """the four loaders of tests/golden/epoch.npz, batches laid out as the reference's DataLoaders yield them"""
    def dl(name, n, width):
        out = []
        for i in range(n):
            x = [g["%s%d_%d" % (name, i, j)] for j in range(width)]
            out.append(tuple(torch.from_numpy(np.asarray(t)) if j < width - 2 else np.asarray(t) for j, t in enumerate(x)))
        return out
    return dl("vt", 2, 8), dl("vv", 1, 8), dl("yt", 2, 6), dl("yv", 1, 6)


def check_epoch_run(pkg, m, g, tmp_path, rtol):
    """run pkg.training_phase on the golden loaders and compare every printed number and the saved checkpoint with what the
    reference's own training_phase (trainer_gmm.py:306-467) printed / saved (tests/golden/make_golden_epoch.py)"""
    import re
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    vt, vv, yt, yv = epoch_loaders(g)
    lines = []
    save_path = os.path.join(str(tmp_path), "golden.pt")
    torch.manual_seed(4242)
    step = pkg.training_phase(tr, int(g["start_step"]), 2, vt, vv, yt, yv, save_path, name="golden", log=lines.append)
    assert step == int(g["start_step"]) + 8
    ref = [str(l) for l in g["lines"]]
    assert len(lines) == len(ref), (lines, ref)
    num = re.compile(r"-?\d+\.\d+")
    for got, want in zip(lines[:-1], ref[:-1]):
        assert num.sub("#", got) == num.sub("#", want), (got, want)              # same text, same number of fields
        a, b = [float(x) for x in num.findall(got)], [float(x) for x in num.findall(want)]
        np.testing.assert_allclose(a, b, rtol=rtol, atol=2e-4, err_msg=want)     # printed with 4-5 decimals
    assert lines[-1].startswith("Model saved as ") and ref[-1].startswith("Model saved as ")
    saved = torch.load(save_path)
    want_keys = [k[len("wend/"):] for k in g.keys() if k.startswith("wend/")]
    assert sorted(saved.keys()) == sorted(want_keys)
    assert all(v.device.type == "cpu" for v in saved.values())
    stamped = [f for f in os.listdir(str(tmp_path)) if f.startswith("golden_") and f.endswith(".pt")]
    assert len(stamped) == 1
    return saved


def make_vae_model(hidden, zdim, device="cpu", ops=None, seed=1234):
    """seeded MusicAttrRegVAE (model_v2.py:9) from the package, on the test backend `ops` (CPU) or the HIP kernels (device)"""
    pkg = load_package()
    torch.manual_seed(seed)
    m = pkg.MusicAttrRegVAE(roll_dims=342, rhythm_dims=3, note_dims=16, chroma_dims=24, hidden_dims=hidden, z_dims=zdim, n_step=20)
    if ops is not None:
        m._make_ops = lambda dev, _ops=ops: _ops          # test-side injection of the CPU stand-in for the kernel table
    return m.to(device)


def check_vae_against_reference(pkg, m, g, dev, rtol_fw, tol_grad, rtol_tuple, atol_w):
    """drop-in forward, fused gradients, three train() steps and evaluate() of the vanilla-VAE sibling vs tests/golden/vae.npz"""
    t = lambda k, dt=None: torch.from_numpy(g[k]).to(dev) if dt is None else torch.from_numpy(g[k]).to(dev).to(dt)
    d, r, n, c = t("d"), t("r"), t("n"), t("c")
    eps = (t("eps_r"), t("eps_n"))
    sd = m.state_dict()
    for k, v in sd.items():
        np.testing.assert_allclose([float(v.double().sum()), float(v.double().abs().sum())], g["w0sum/" + k], rtol=1e-6, atol=1e-6, err_msg=k)
    assert set(sd) == {k[len("w0sum/"):] for k in g if k.startswith("w0sum/")}
    # drop-in forward: the reference's nested tuple (model_v2.py:165-171)
    (out, r_out, n_out), (dis_r, dis_n), (z_r, z_n) = m(pkg.convert_to_one_hot(d, 342), pkg.convert_to_one_hot(r, 3), pkg.convert_to_one_hot(n, 16), c, eps=eps)
    got = dict(out=out, r_out=r_out, n_out=n_out, mu_r=dis_r.mean, sigma_r=dis_r.stddev, mu_n=dis_n.mean, sigma_n=dis_n.stddev, z_r=z_r, z_n=z_n)
    for k, v in got.items():
        np.testing.assert_allclose(v.detach().cpu().numpy(), g["fw_" + k], rtol=rtol_fw, atol=rtol_fw, err_msg=k)
    # fused step
    tr = pkg.VAETrainer(m, lr=1e-3, beta=0.1)
    batch = tr.prepare_batch(g["d"], g["r"], g["n"], g["c"], g["r_density"], g["n_density"])
    tup = tr.loss_and_grads(5000, batch, eps)
    np.testing.assert_allclose(tup[:6], g["loss_terms"], rtol=rtol_tuple)
    for k in tr.flat.names:
        ref = g["grad/" + k]
        e = relerr(tr.flat.G[k].cpu().numpy(), ref)
        assert e < tol_grad or np.abs(ref).max() < 1e-6, (k, e)
    assert set(tr.flat.names) == {k[len("grad/"):] for k in g if k.startswith("grad/")}
    np.testing.assert_allclose(tr.grad_norm(), g["gradnorm"][0], rtol=1e-3)
    step = 5000
    for it in range(3):
        torch.manual_seed(99 + it)
        step, tup = tr.train(step, None, None, None, g["d"], g["r"], g["n"], g["c"], g["r_density"], g["n_density"])
        assert len(tup) == 6
        np.testing.assert_allclose(tup, g["train_tuples"][it], rtol=rtol_tuple, err_msg="step %d" % it)
    assert step == 5003
    torch.manual_seed(123)
    ev = tr.evaluate(None, None, None, g["d"], g["r"], g["n"], g["c"], g["r_density"], g["n_density"])
    np.testing.assert_allclose(ev, g["eval_tuple"], rtol=rtol_tuple)
    for k, v in m.state_dict().items():
        if k not in NOISE_PARAMS:
            np.testing.assert_allclose(v.cpu().numpy(), g["w3/" + k], rtol=0, atol=atol_w, err_msg=k)


def tokens_match_upto_near_tie(tok, ref_tok, ref_gap, thr=1e-4):
    """greedy tokens are compared per row up to the first position where the reference's own top-2 log-prob gap is below thr
    (a flipped float32 near-tie changes every later token); returns the number of positions compared"""
    tok, ref_tok = np.asarray(tok), np.asarray(ref_tok)
    L = tok.shape[-1]
    n = 0
    for row, rrow, grow in zip(tok.reshape(-1, L), ref_tok.reshape(-1, L), np.asarray(ref_gap).reshape(-1, L)):
        unclear = np.where(grow < thr)[0]
        upto = int(unclear[0]) if len(unclear) else L
        assert np.array_equal(row[:upto], rrow[:upto]), (row[:upto].tolist(), rrow[:upto].tolist())
        n += upto
    return n


REPLAY_ROWS = 256          # rows replayed per decode above this batch size: a fixed-seed sample (decode rows are independent)
REPLAY_BLOCK = 32          # pipeline blocks (32 / 64 rows) and cell row tiles (multiples of 64 / 128 rows) all start at multiples of 32
REPLAY_CAP = 0.02          # at most this share of the checked positions may sit at an fp64 top-2 gap below delta
_DECODER_KEYS = ("linear_init_global.", "grucell_g.", "grucell_g_2.", "linear_out_g.")


def replay_rows(Bi, n=REPLAY_ROWS, seed=0):
    """every row when Bi <= n; else n rows drawn with a fixed seed that include the first and last row of every 32-row block (so of every
    32- / 64-row pipeline block and every cell row tile) and the last row of the batch"""
    if Bi <= n:
        return np.arange(Bi)
    must = set()
    for r0 in range(0, Bi, REPLAY_BLOCK):
        must.update((r0, min(r0 + REPLAY_BLOCK, Bi) - 1))
    must.add(Bi - 1)
    assert len(must) <= n
    rest = np.setdiff1d(np.arange(Bi), np.fromiter(must, dtype=np.int64))
    extra = np.random.RandomState(seed).choice(rest, n - len(must), replace=False)
    return np.sort(np.concatenate([np.fromiter(must, dtype=np.int64), extra]))


def replay_decode_check(sd, z, tokens, logp=None, rows=None):
    """Every step of a greedy decode against an fp64 replay of its own tokens.

    Step i of the greedy decoder consumes token i-1, which is what the teacher-forced oracle decoder does with teacher=tokens: replaying
    the tokens a kernel chose gives the exact log-probs it should have computed at every position, whatever it chose earlier.  The
    tokens are replayed twice: in fp64 (the reference) and in fp32 (the plain CPU restatement), whose distance e_ref = max |lp32 - lp64|
    is what fp32 rounding alone costs on these inputs.  tol_lp = min(1e-4, 16 e_ref): 1e-4 is the absolute tolerance the suite already
    applies to these paths against the oracle, 16 is headroom for the kernels' other summation orders (split-K partials through LDS,
    bf16 x 6 products whose dropped terms are fp32-class).  At every replayed position:
      (a) logp given: |lp_gpu - lp64| <= tol_lp over all 342 entries;
      (b) logp given: the token is the first-index argmax of the kernel's own log-prob row;
      (c) lp64[tok] >= max(lp64) - delta, delta = 2 tol_lp (log-prob differences are logit differences, each side off by at most tol_lp):
          wherever the fp64 top-2 gap exceeds delta the token IS the fp64 argmax.
    And a condition on the inputs: at most 2 % of the positions have an fp64 top-2 gap below delta (only there is a token unconstrained).
    sd: the model's state dict; z (Bi, 2Z+24); tokens (Bi, steps); logp (Bi, steps, 342) or None; rows: indices or None (replay_rows).
    Returns the figures as a dict."""
    t0 = time.time()
    tokens = torch.as_tensor(tokens).detach().cpu().long()
    Bi, steps = tokens.shape
    rows = torch.as_tensor(replay_rows(Bi) if rows is None else rows, dtype=torch.long)
    tk = tokens[rows]
    E = orc.E
    assert int(tk.min()) >= 0 and int(tk.max()) < E, ("token out of range", int(tk.min()), int(tk.max()))
    zr = torch.as_tensor(z).detach().cpu()[rows]
    dec = {k: v.detach().cpu() for k, v in sd.items() if k.startswith(_DECODER_KEYS)}
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))         # what a GPU machine allows a test
    try:
        with torch.no_grad():
            lp64 = orc.global_decoder({k: v.double() for k, v in dec.items()}, zr.double(), steps, teacher=tk)
            lp32 = orc.global_decoder({k: v.float() for k, v in dec.items()}, zr.float(), steps, teacher=tk)
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
              max_dlp=float("nan"), ratio=float("nan"))

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


# the decode cases test_gpu_parity.test_decode_paths_every_step_vs_fp64_replay forces, (path, weights, Bi, steps):
#   one_launch  fn_decode_greedy, one block of <= 32 rows        pipeline32 / pipeline64  its block pipeline, 32- / 64-row blocks
#   scan_steps  per-token scan-step kernels + projection GEMM     cells_f32 / cells_x6     per-token fn_gru_cell_f32 cells, fp32 / bf16 x 6
# the graph paths (scan_steps, cells_*) also replay their cached graph on a second latent batch (seed Bi + 1)
REPLAY_CASES = [
    ("one_launch", "h64", 1, 300), ("one_launch", "h64", 17, 300), ("one_launch", "h64", 32, 300),
    ("one_launch", "h512", 1, 300), ("one_launch", "h512", 17, 300), ("one_launch", "h512", 32, 300),
    ("pipeline32", "h512", 33, 300), ("pipeline32", "h64", 200, 250), ("pipeline32", "h512", 352, 200),
    ("pipeline64", "h512", 353, 150), ("pipeline64", "h512", 704, 300), ("pipeline64", "h64", 1500, 120), ("pipeline64", "h512", 2048, 100),
    ("scan_steps", "h64", 17, 300), ("scan_steps", "h512", 300, 150),
    ("cells_f32", "h512", 705, 200), ("cells_f32", "h512", 1000, 150), ("cells_f32", "h512", 1280, 120),
    ("cells_x6", "h512", 2048, 300),
    ("pipeline32", "trained64", 40, 300),
]
REPLAY_GRAPH_PATHS = ("scan_steps", "cells_f32", "cells_x6")
# the row blocks of the one-launch kernel a case's name stands for: (rows of a block, blocks) of Bi sequences - one block of 16 or 32 rows, a pipeline of
# 32-row blocks, a pipeline of 64-row blocks; compared with what the library plans for the case's tensors (fn_decode_plan)
ONE_LAUNCH_BLOCKS = {"one_launch": lambda Bi: (16 if Bi <= 16 else 32, 1), "pipeline32": lambda Bi: (32, -(-Bi // 32)), "pipeline64": lambda Bi: (64, -(-Bi // 64))}
REPLAY_OUT_SCALE = 8.0     # linear_out_g.weight x 8: wider logit spreads, fewer near-ties (seeded H=512: 1.8 % of the gaps below 2e-4 -> 0.4 %)


def replay_inputs(weights):
    """(H, Z, state dict) of a replay case, on the CPU: 'h64' / 'h512' = the seeded model (seed 7 / 1234) with linear_out_g.weight x 8,
    'trained64' = the trained weights tests/golden/epoch.npz ends with (wend/), unscaled"""
    if weights == "trained64":
        sd = sd_from(load_golden("epoch"), "wend/")
    else:
        H = int(weights[1:])
        m = make_model(H, 32 if H == 64 else 128, seed=7 if H == 64 else 1234)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        sd["linear_out_g.weight"] = sd["linear_out_g.weight"] * REPLAY_OUT_SCALE
    H, Zc = sd["linear_init_global.weight"].shape
    return int(H), (int(Zc) - 24) // 2, sd


def replay_z(Bi, Z, seed):
    """the latent rows of a replay case: N(0, 1), (Bi, 2Z + 24), from their own generator"""
    return torch.randn(Bi, 2 * Z + 24, generator=torch.Generator().manual_seed(seed))


def replay_line(path, H, st):
    """one line of profiles/decode_replay_errors.txt"""
    return ("%-26s Bi %4d H %3d steps %3d rows %3d  e_ref %.3e  max|dlogp| %.3e  ratio %6.3f  below_delta %.3f %%  delta %.3e  replay %.1f s"
            % (path, st["Bi"], H, st["steps"], st["rows"], st["e_ref"], st["max_dlp"], st["ratio"], 100 * st["share_below_delta"], st["delta"],
               st["seconds"]))


def eval_golden(tag):
    return {k[len(tag) + 1:]: v for k, v in load_golden("eval").items() if k.startswith(tag + "/")}


def check_eval_side(pkg, m, g, dev, rtol=2e-5):
    """the product's eval-side callers (evaluators.py, eval-mode forward, fader_sweep) against tests/golden/eval.npz = the reference's
    own evaluator / notebook code run on the same seeds (make_golden_eval.py).  `m` is a freshly seeded model on `dev`."""
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    d, r, n, c = t("d"), t("r"), t("n"), t("c")
    B, T = d.shape
    Z = m.latent_dim
    for k, v in m.state_dict().items():
        np.testing.assert_allclose([float(v.double().sum())], g["w0sum/" + k][:1], rtol=1e-9, atol=1e-9, err_msg=k)
    # D: run_through_gmm (train mode as constructed)
    m.train()
    dl = [(d[i:i + 3], r[i:i + 3], n[i:i + 3], c[i:i + 3], g["r_density"][i:i + 3], g["n_density"][i:i + 3]) for i in range(0, B, 3)]
    torch.manual_seed(5)
    res = pkg.run_through_gmm(m, dl)
    names = ["r_density_lst", "n_density_lst", "r_lst", "n_lst", "a_lst", "r_mean", "n_mean", "z_r_0_lst", "z_r_rest_lst",
             "z_n_0_lst", "z_n_rest_lst", "r_min", "r_max", "n_min", "n_max"]
    for k, v in zip(names, res):
        if k != "a_lst":
            np.testing.assert_allclose(np.asarray(v), g["rt_" + k], rtol=rtol, atol=rtol, err_msg=k)
    # B: evaluator shifts, the reference's call sequence: the first call finds the model in train mode, later ones in eval mode
    m.train()
    ev = {0: pkg.GMMRhythmEvaluator(None), 1: pkg.GMMNoteEvaluator(None)}
    compared = 0
    for k, (which, i, val) in enumerate(g["shift_calls"]):
        i = int(i)
        assert m.training == bool(g["shift%d_training_before" % k][0])
        torch.manual_seed(100 + k)
        out, z0 = ev[int(which)].shift(m, d[i], r[i], n[i], c[i], float(val))
        assert tuple(out.shape) == (1, 100, 342) and not m.training
        np.testing.assert_allclose(z0, g["shift%d_z0" % k][0], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(out[0, 0].cpu().numpy(), g["shift%d_logp0" % k], rtol=1e-4, atol=1e-4)
        compared += tokens_match_upto_near_tie(out.argmax(-1).cpu().numpy(), g["shift%d_tokens" % k], g["shift%d_gap" % k])
        if (g["shift%d_gap" % k] >= 1e-4).all():
            assert np.array_equal(np.asarray(pkg.clean_output(out)), g["shift%d_clean" % k])
    assert compared >= 100
    # the batched form of the same shifts: (sample, value) rows of one decode batch, eps per (sample, value)
    for which in (0, 1):
        calls = [(k, int(i), float(v)) for k, (w, i, v) in enumerate(g["shift_calls"]) if int(w) == which]
        # the reference call k draws [forward eps r, n (+T rand)] then repar r, n: reproduce the repar draws
        eps_r, eps_n = torch.zeros(B, len(calls), Z), torch.zeros(B, len(calls), Z)
        for j, (k, i, v) in enumerate(calls):
            torch.manual_seed(100 + k)
            torch.randn(1, Z), torch.randn(1, Z)
            if bool(g["shift%d_training_before" % k][0]):
                for _ in range(T):
                    torch.rand(1)
            eps_r[i, j], eps_n[i, j] = torch.randn(1, Z)[0], torch.randn(1, Z)[0]
        tk, z0 = pkg.fader_sweep(m, d, c, [v for _, _, v in calls], steps=100, which="rn"[which], eps=(eps_r, eps_n))
        assert tuple(tk.shape) == (B, len(calls), 100) and tuple(z0.shape) == (B, len(calls))
        for j, (k, i, v) in enumerate(calls):
            np.testing.assert_allclose(float(z0[i, j]), g["shift%d_z0" % k][0], rtol=1e-4, atol=1e-5)
            tokens_match_upto_near_tie(tk[i, j].cpu().numpy()[None], g["shift%d_tokens" % k], g["shift%d_gap" % k])
    # A: eval-mode forward: the decoder feeds back its own argmax, no rand(1) draws
    m.eval()
    torch.manual_seed(7)
    (o, r_out, n_out, _, _), dis, z_out, ll_out, qy_out, y_out = m(pkg.convert_to_one_hot(d, 342), pkg.convert_to_one_hot(r, 3),
                                                                   pkg.convert_to_one_hot(n, 16), c)
    after = torch.rand(1).item()
    torch.manual_seed(7)
    torch.randn(B, Z), torch.randn(B, Z)
    assert after == torch.rand(1).item()
    got = dict(r_out=r_out, n_out=n_out, mu_r=dis[0].mean, sigma_r=dis[0].stddev, z_r=z_out[0], z_n=z_out[1], ll_r=ll_out[0], qy_n=qy_out[1])
    for k, v in got.items():
        np.testing.assert_allclose(v.cpu().numpy(), g["evalfw_" + k], rtol=rtol, atol=rtol, err_msg=k)
    np.testing.assert_allclose(o[:, 0].cpu().numpy(), g["evalfw_logp0"], rtol=1e-4, atol=1e-4)
    assert tuple(o.shape) == (B, T, 342)
    assert tokens_match_upto_near_tie(o.argmax(-1).cpu().numpy(), g["evalfw_tokens"], g["evalfw_gap"]) >= B * T // 2
    assert np.array_equal(y_out[0].cpu().numpy(), g["evalfw_y_r"]) and np.array_equal(y_out[1].cpu().numpy(), g["evalfw_y_n"])
    # C: notebook transfer (cells 11 + 15 / 17), 300 greedy steps, both latents shifted
    for j in range(2):
        i, seed, lmbda, steps = (int(x) for x in g["nb%d_meta" % j])
        torch.manual_seed(seed)
        out, z = pkg.arousal_transfer(m, d[i], c[i], lmbda=lmbda, low_to_high=(j == 0), steps=steps)
        assert tuple(out.shape) == (1, 300, 342)
        np.testing.assert_allclose(z.cpu().numpy(), g["nb%d_z" % j], rtol=1e-4, atol=1e-5)
        assert tokens_match_upto_near_tie(out.argmax(-1).cpu().numpy(), g["nb%d_tokens" % j], g["nb%d_gap" % j]) >= 100
        # and its batched form: mode="shift", which="both", lambda = +-1
        torch.manual_seed(seed)
        eps = (torch.randn(1, Z), torch.randn(1, Z))
        tk, _ = pkg.fader_sweep(m, d[i:i + 1], c[i:i + 1], [lmbda if j == 0 else -lmbda], steps=steps, which="both", mode="shift", eps=eps)
        tokens_match_upto_near_tie(tk[0].cpu().numpy(), g["nb%d_tokens" % j], g["nb%d_gap" % j])
    # train-mode global_decoder(z, steps): teacher forced with self.sample (gmm_model.py:139-142)
    m.train()
    torch.manual_seed(11)
    (o_tf, _, _, _, _), _, z_out, _, _, _ = m(d, r, n, c)
    zc = torch.cat([z_out[0], z_out[1], c], dim=1).detach()
    o2 = m.global_decoder(zc, steps=T)
    assert o2.requires_grad                                      # as in the reference: a train-mode call is part of the autograd graph
    np.testing.assert_allclose(o2.detach().cpu().numpy(), o_tf.detach().cpu().numpy(), rtol=1e-5, atol=1e-5)


# ---- single-encoder siblings (tests/golden/siblings.npz = the reference's model_v2 classes + their own trainers) ----------------------
SIBLINGS = {"single": ("MusicAttrSingleVAE", "SingleVAETrainer"), "cvae": ("MusicAttrCVAE", "CVAETrainer"), "fader": ("MusicAttrFaderNets", "FaderTrainer")}


def sibling_golden(kind):
    return {k[len(kind) + 1:]: v for k, v in load_golden("siblings").items() if k.startswith(kind + "/")}


def make_sibling(kind, hidden, zdim, device="cpu", ops=None, seed=1234):
    pkg = load_package()
    torch.manual_seed(seed)
    m = getattr(pkg, SIBLINGS[kind][0])(roll_dims=342, rhythm_dims=3, note_dims=16, chroma_dims=24, hidden_dims=hidden, z_dims=zdim, n_step=20)
    if ops is not None:
        m._make_ops = lambda dev, _ops=ops: _ops          # test-side injection of the CPU stand-in for the kernel table
    return m.to(device)


def check_sibling(pkg, kind, m, g, dev, rtol_fw=5e-5, tol_grad=5e-4, rtol_tuple=5e-4):
    """drop-in forward (train and eval mode), fused gradients, three train() steps and evaluate() of one sibling against the reference run"""
    H, Z, B, T, Tr = (int(x) for x in g["dims"])
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    d, r, n, c = t("d"), t("r"), t("n"), t("c")
    rd32, nd32 = torch.from_numpy(g["r_density"]).float().unsqueeze(-1).to(dev), torch.from_numpy(g["n_density"]).float().unsqueeze(-1).to(dev)
    for k, v in m.state_dict().items():
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), vd.abs().sum().item(), (vd * vd).sum().item()], g["w0sum/" + k], rtol=1e-9, atol=1e-9, err_msg=k)
    assert set(m.state_dict()) == {k[len("w0sum/"):] for k in g if k.startswith("w0sum/")}
    call = (lambda: m(pkg.convert_to_one_hot(d, 342), c)) if kind == "single" else \
           (lambda: m(pkg.convert_to_one_hot(d, 342), pkg.convert_to_one_hot(r, 3), pkg.convert_to_one_hot(n, 16), c, rd32, nd32))
    # train-mode forward, the reference's nesting, random draws from the seeded global generator
    m.train()
    torch.manual_seed(99)
    res = call()
    if kind == "fader":
        (o, r_out, n_out), dis, z = res
        np.testing.assert_allclose(r_out.detach().cpu().numpy(), g["fw_r_out"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(n_out.detach().cpu().numpy(), g["fw_n_out"], rtol=1e-4, atol=1e-5)
    else:
        o, dis, z = res
    assert o.requires_grad                                        # a train-mode call is part of the autograd graph, as in the reference
    for k, v in (("out", o), ("mu", dis.mean), ("sigma", dis.stddev), ("z", z)):
        np.testing.assert_allclose(v.detach().cpu().numpy(), g["fw_" + k], rtol=rtol_fw, atol=rtol_fw, err_msg=k)
    # fused gradients
    tr = getattr(pkg, SIBLINGS[kind][1])(m, lr=1e-3, beta=0.2)
    batch = tr.prepare_batch(g["d"], g["r"], g["n"], g["c"], g["r_density"], g["n_density"])
    for step in ((20000, 500) if kind == "fader" else (20000,)):
        torch.manual_seed(99)
        eps = tr.draw_eps(B, T)
        tup = tr.loss_and_grads(step, batch, eps)
        np.testing.assert_allclose(tup, g["loss_terms_%d" % step], rtol=rtol_tuple, atol=1e-9)
        ref_keys = {k[len("grad_%d/" % step):] for k in g if k.startswith("grad_%d/" % step)}
        assert set(tr.flat.names) == ref_keys, (set(tr.flat.names) ^ ref_keys)
        for k in tr.flat.names:
            ref = g["grad_%d/%s" % (step, k)]
            e = relerr(tr.flat.G[k].cpu().numpy(), ref)
            assert e < tol_grad or np.abs(ref).max() < 1e-7, (kind, step, k, e)
        np.testing.assert_allclose(tr.grad_norm(), g["gradnorm_%d" % step][0], rtol=1e-3)
    # the reference's own train() x3 and evaluate()
    step = 19999
    for it in range(3):
        torch.manual_seed(99 + it)
        # the densities as the reference's own loops hand them over: float64 arrays (trainer_singlevae.py:107-120), (B, 1) float32
        # device tensors for the conditional models (trainer_cvae.py:171, trainer_fader.py:180)
        dens = (g["r_density"], g["n_density"]) if kind == "single" or it == 2 else (rd32, nd32)
        step, tup = tr.train(step, None, None, None, g["d"], g["r"], g["n"], g["c"], *dens)
        np.testing.assert_allclose(tup, g["train_tuples"][it], rtol=rtol_tuple, atol=1e-9, err_msg="step %d" % it)
    assert step == 20002
    for k, v in m.state_dict().items():
        vd = v.double()
        np.testing.assert_allclose([vd.abs().sum().item()], g["w3sum/" + k][1:2], rtol=1e-3, err_msg=k)
    torch.manual_seed(123)
    if kind == "cvae":
        ev = tr.evaluate(None, None, None, g["d"], g["r"], g["n"], g["c"], rd32, nd32)
    elif kind == "fader":
        ev = tr.evaluate(step - 1, None, None, None, g["d"], g["r"], g["n"], g["c"], rd32, nd32)
    else:
        ev = tr.evaluate(step - 1, None, None, None, g["d"], g["r"], g["n"], g["c"], g["r_density"], g["n_density"])
    np.testing.assert_allclose(ev, g["eval_tuple"], rtol=rtol_tuple, atol=1e-9)
    # eval-mode forward on fresh weights: greedy decoder
    m2 = make_sibling(kind, H, Z, device=dev, ops=m._make_ops(None) if "_make_ops" in m.__dict__ else None)
    m2.eval()
    d, r, n, c = (x.to(dev) for x in (d, r, n, c))
    torch.manual_seed(7)
    res = (m2(pkg.convert_to_one_hot(d, 342), c) if kind == "single" else
           m2(pkg.convert_to_one_hot(d, 342), pkg.convert_to_one_hot(r, 3), pkg.convert_to_one_hot(n, 16), c, rd32, nd32))
    o = res[0][0] if kind == "fader" else res[0]
    np.testing.assert_allclose(res[2].cpu().numpy(), g["evalfw_z"], rtol=rtol_fw, atol=rtol_fw)
    np.testing.assert_allclose(o[:, 0].cpu().numpy(), g["evalfw_logp0"], rtol=1e-4, atol=1e-4)
    assert tokens_match_upto_near_tie(o.argmax(-1).cpu().numpy(), g["evalfw_tokens"], g["evalfw_gap"]) >= B * T // 2
    if kind == "fader":
        np.testing.assert_allclose(res[0][1].cpu().numpy(), g["evalfw_r_out"], rtol=1e-4, atol=1e-5)


# ---- GLSR trainer (tests/golden/glsr.npz = trainer_glsr.py's own functions on model_v2.MusicAttrRegVAE) ---------------------------------
def glsr_fixture_weights(g, hidden, zdim):
    """the seeded MusicAttrRegVAE weights with the fixture's output-layer modification (make_golden_glsr.py)"""
    from oracle import vae_oracle as vo
    sd = vo.init_state_dict(hidden, zdim)
    sd["linear_out_g.weight"] = sd["linear_out_g.weight"] * float(g["out_scale"][0])
    sd["linear_out_g.bias"] = sd["linear_out_g.bias"] + torch.from_numpy(g["bias_shift"])
    for k, v in sd.items():
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), vd.abs().sum().item(), (vd * vd).sum().item()], g["w0sum/" + k], rtol=1e-6, atol=1e-6, err_msg=k)
    return sd


def check_glsr(pkg, m, g, dev, tol_grad=1e-3, rtol_tuple=5e-4):
    """GLSRTrainer (fused step + four extra teacher-forced decodes + host walk) vs the reference's trainer_glsr.train / evaluate"""
    H, Z, B, T, Tr = (int(x) for x in g["dims"])
    tr = pkg.GLSRTrainer(m, lr=1e-3, beta=0.2)
    batch = tr.prepare_batch(g["d"], g["r"], g["n"], g["c"], g["r_density"], g["n_density"])
    torch.manual_seed(99)
    eps = tr.draw_eps(B, T, step=20000)
    assert len(eps[2]) == 2
    tup = tr.loss_and_grads(20000, batch, eps)[:6]
    np.testing.assert_allclose(tup, g["loss_terms_20000"], rtol=rtol_tuple)
    assert tup[5] > 0.92 and float(g["diag_sep_frac_above"][0]) > 0.2          # the regulariser is not at its constant floor
    ref_keys = {k[len("grad/"):] for k in g if k.startswith("grad/")}
    assert set(tr.flat.names) == ref_keys
    for k in tr.flat.names:
        ref = g["grad/" + k]
        e = relerr(tr.flat.G[k].cpu().numpy(), ref)
        assert e < tol_grad or np.abs(ref).max() < 1e-6, (k, e)
    np.testing.assert_allclose(tr.grad_norm(), g["gradnorm"][0], rtol=2e-3)
    # step <= 20: regulariser off, no extra draws (trainer_glsr.py:289-292)
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(50)
    _, t19 = tr.train(19, None, None, None, g["d"], g["r"], g["n"], g["c"], g["r_density"], g["n_density"])
    np.testing.assert_allclose(t19, g["train_tuple_step19"], rtol=rtol_tuple, atol=1e-9)
    # the reference's own train() x3 from the fixture weights, then evaluate()
    m.load_state_dict(sd0)
    tr = pkg.GLSRTrainer(m, lr=1e-3, beta=0.2)
    step = 19999
    for it in range(3):
        torch.manual_seed(99 + it)
        step, tup = tr.train(step, None, None, None, g["d"], g["r"], g["n"], g["c"], g["r_density"], g["n_density"])
        np.testing.assert_allclose(tup, g["train_tuples"][it], rtol=2e-3 if it else rtol_tuple, err_msg="step %d" % it)
    torch.manual_seed(123)
    ev = tr.evaluate(step - 1, None, None, None, g["d"], g["r"], g["n"], g["c"], g["r_density"], g["n_density"])
    np.testing.assert_allclose(ev, g["eval_tuple"], rtol=2e-3)


# ---- autograd through DIRECT sub-module calls (encode / sub_decoders / global_decoder / approx_qy_x, gmm_model.py:82-218) -----------------
def check_direct_call_autograd(pkg, m, g, dev, tol=5e-4):
    """each direct call in train mode is one autograd node: values and the gradients wrt inputs / parameters against torch autograd of the
    oracle's restatement of the same reference lines, on the `small` fixture's weights and batch"""
    from oracle import gmvae_oracle as orc
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    b = batch_of(g)
    d, r, n = (torch.from_numpy(b[k]) for k in ("d", "r", "n"))
    B, T = d.shape
    Z = m.latent_dim
    m.train()

    def leaves(keys):
        return {k: sd[k].clone().requires_grad_(True) for k in keys}

    def cmp(got, ref, what):
        got, ref = got.detach().cpu().double().numpy(), ref.detach().double().numpy()
        scale = max(1e-6, float(np.abs(ref).max()))
        assert float(np.abs(got - ref).max()) <= tol * scale, (what, float(np.abs(got - ref).max()), scale)

    def zero_grads():
        for p in m.parameters():
            p.grad = None

    # ---- encode ------------------------------------------------------------------------------------------------------
    torch.manual_seed(1)
    w = [torch.randn(B, Z) for _ in range(4)]
    keys = [k for k in sd if k.startswith(("gru_r.", "gru_n.", "mu_r.", "var_r.", "mu_n.", "var_n."))]
    L = leaves(keys)
    p = dict(sd); p.update(L)
    ref = orc.encode(p, orc.convert_to_one_hot(d, 342))
    gref = torch.autograd.grad(sum((o * wi).sum() for o, wi in zip(ref, w)), [L[k] for k in keys])
    zero_grads()
    dis_r, dis_n = m.encode(pkg.convert_to_one_hot(d.to(dev), 342))
    got = (dis_r.mean, dis_r.stddev, dis_n.mean, dis_n.stddev)
    for o, ro, nm in zip(got, ref, ("mu_r", "sigma_r", "mu_n", "sigma_n")):
        cmp(o, ro, "encode " + nm)
    sum((o * wi.to(dev)).sum() for o, wi in zip(got, w)).backward()
    params = dict(m.named_parameters())
    for k, gr in zip(keys, gref):
        cmp(params[k].grad, gr, "encode grad " + k)
    assert params["linear_out_g.weight"].grad is None

    # ---- sub_decoders ----------------------------------------------------------------------------------------------------
    torch.manual_seed(2)
    z_r, z_n = torch.randn(B, Z) * 0.5, torch.randn(B, Z) * 0.5
    keys = [k for k in sd if k.startswith(("gru_d_r.", "gru_d_n.", "linear_out_r.", "linear_out_n.", "linear_init_r.", "linear_init_n."))]
    L = leaves(keys)
    p = dict(sd); p.update(L)
    zr_l, zn_l = z_r.clone().requires_grad_(True), z_n.clone().requires_grad_(True)
    ref_r = orc.sub_decoder(p, "r", orc.convert_to_one_hot(r, 3), zr_l)
    ref_n = orc.sub_decoder(p, "n", orc.convert_to_one_hot(n, 16), zn_l)
    wr, wn = torch.randn_like(ref_r), torch.randn_like(ref_n)
    gref = torch.autograd.grad((ref_r * wr).sum() + (ref_n * wn).sum(), [zr_l, zn_l] + [L[k] for k in keys])
    zero_grads()
    zr_d, zn_d = z_r.to(dev).requires_grad_(True), z_n.to(dev).requires_grad_(True)
    r_out, n_out, _, _ = m.sub_decoders(pkg.convert_to_one_hot(r.to(dev), 3), zr_d, pkg.convert_to_one_hot(n.to(dev), 16), zn_d)
    cmp(r_out, ref_r, "sub_decoders r_out"), cmp(n_out, ref_n, "sub_decoders n_out")
    ((r_out * wr.to(dev)).sum() + (n_out * wn.to(dev)).sum()).backward()
    cmp(zr_d.grad, gref[0], "sub_decoders dz_r"), cmp(zn_d.grad, gref[1], "sub_decoders dz_n")
    for k, gr in zip(keys, gref[2:]):
        if k in ("linear_out_r.bias", "linear_out_n.bias"):       # mathematically zero (time-axis softmax): rounding noise on both sides
            continue
        cmp(params[k].grad, gr, "sub_decoders grad " + k)

    # ---- global_decoder (train mode: teacher forced with self.sample) --------------------------------------------------
    torch.manual_seed(3)
    steps = T - 3
    zc = torch.randn(B, 2 * Z + 24) * 0.5
    keys = [k for k in sd if k.startswith(("linear_out_g.", "grucell_g_2.", "grucell_g.", "linear_init_global."))]
    L = leaves(keys)
    p = dict(sd); p.update(L)
    zc_l = zc.clone().requires_grad_(True)
    teacher = d.long()[:, :steps]
    ref = orc.global_decoder(p, zc_l, steps, teacher=teacher)
    wo = torch.randn_like(ref)
    gref = torch.autograd.grad((ref * wo).sum(), [zc_l] + [L[k] for k in keys])
    zero_grads()
    m.sample = pkg.convert_to_one_hot(d.to(dev), 342)
    zc_d = zc.to(dev).requires_grad_(True)
    state = torch.get_rng_state()
    out = m.global_decoder(zc_d, steps)
    torch.set_rng_state(state)
    for _ in range(steps):
        torch.rand(1)
    probe = torch.rand(1)
    cmp(out, ref, "global_decoder out")
    (out * wo.to(dev)).sum().backward()
    cmp(zc_d.grad, gref[0], "global_decoder dz")
    for k, gr in zip(keys, gref[1:]):
        cmp(params[k].grad, gr, "global_decoder grad " + k)
    assert probe.numel() == 1                                     # (the call drew `steps` x rand(1), as the reference does)

    # ---- approx_qy_x -----------------------------------------------------------------------------------------------------
    torch.manual_seed(4)
    z = (torch.randn(B, Z) * 0.3)
    z_l = z.clone().requires_grad_(True)
    mu_l = sd["mu_r_lookup.weight"].clone().requires_grad_(True)
    ll_ref, qy_ref = orc.approx_qy_x(z_l, mu_l, sd["logvar_r_lookup.weight"])
    w1, w2 = torch.randn_like(ll_ref) * 1e-2, torch.randn_like(qy_ref)
    gref = torch.autograd.grad((ll_ref * w1).sum() + (qy_ref * w2).sum(), [z_l, mu_l])
    zero_grads()
    z_d = z.to(dev).requires_grad_(True)
    ll, qy = m.approx_qy_x(z_d, m.mu_r_lookup, m.logvar_r_lookup, m.n_component)
    cmp(ll, ll_ref, "approx_qy_x ll")
    ((ll * w1.to(dev)).sum() + (qy * w2.to(dev)).sum()).backward()
    cmp(z_d.grad, gref[0], "approx_qy_x dz")
    cmp(m.mu_r_lookup.weight.grad, gref[1], "approx_qy_x dmu_lookup")
    # stale backward is refused; eval mode / no_grad stay forward only
    o1 = m.encode(d.to(dev))[0].mean
    m.encode(d.to(dev))
    try:
        o1.sum().backward()
        raise AssertionError("stale backward accepted")
    except RuntimeError as e:
        assert "must run before the next" in str(e)
    with torch.no_grad():
        assert not m.encode(d.to(dev))[0].mean.requires_grad
    m.eval()
    assert not m.encode(d.to(dev))[0].mean.requires_grad
    m.train()


def check_sibling_autograd(pkg, kind, m, g, dev, tol_grad=5e-4):
    """the reference's own training pattern on the single-encoder drop-ins: forward in train mode, the trainer script's loss written with
    torch ops on the returned tensors (trainer_singlevae.py:87-120, trainer_cvae.py:87-103, trainer_fader.py:87-110), loss.backward() - the
    parameter gradients must be the reference's (siblings.npz grad_20000/*)"""
    from torch.distributions import Normal, kl_divergence
    H, Z, B, T, Tr = (int(x) for x in g["dims"])
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    d, r, n, c = t("d"), t("r"), t("n"), t("c")
    rd32, nd32 = torch.from_numpy(g["r_density"]).float().unsqueeze(-1).to(dev), torch.from_numpy(g["n_density"]).float().unsqueeze(-1).to(dev)
    m.train()
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(99)
    if kind == "single":
        out, dis, z = m(pkg.convert_to_one_hot(d, 342), c)
    else:
        res = m(pkg.convert_to_one_hot(d, 342), pkg.convert_to_one_hot(r, 3), pkg.convert_to_one_hot(n, 16), c, rd32, nd32)
        (out, r_out, n_out), dis, z = res if kind == "fader" else ((res[0], None, None), res[1], res[2])
    assert out.requires_grad and dis.mean.requires_grad and z.requires_grad
    step, beta = 20000, 0.2
    ce = torch.nn.functional.nll_loss(out.reshape(-1, out.shape[-1]), d.reshape(-1).long())
    kld = kl_divergence(dis, Normal(torch.zeros_like(dis.mean), torch.ones_like(dis.stddev))).mean()
    beta0 = 0.0 if step < 1000 else min((step - 10000) / 10000 * beta, beta)
    if kind == "single":
        regs = []
        for col, a in ((0, g["r_density"]), (1, g["n_density"])):
            da = torch.from_numpy(np.subtract.outer(np.asarray(a, np.float64), np.asarray(a, np.float64))).float().to(dev)
            zc = z[:, col]
            regs.append(((torch.tanh(zc.reshape(-1, 1) - zc) - torch.sign(da)) ** 2).mean())
        loss = 5 * ce + beta * kld + regs[0] + regs[1]
    elif kind == "cvae":
        loss = ce + beta0 * kld
    else:
        lam = min(step / 2000 * 1e-4, 1e-4)
        loss = ce + beta0 * kld + lam * torch.nn.functional.mse_loss(r_out, rd32) + lam * torch.nn.functional.mse_loss(n_out, nd32)
    np.testing.assert_allclose(float(loss.detach()), g["loss_terms_20000"][0], rtol=5e-4)
    loss.backward()
    params = dict(m.named_parameters())
    seen = 0
    for k in [k[len("grad_20000/"):] for k in g if k.startswith("grad_20000/")]:
        ref = g["grad_20000/" + k]
        assert params[k].grad is not None, k
        e = relerr(params[k].grad.cpu().numpy(), ref)
        assert e < tol_grad or np.abs(ref).max() < 1e-7, (kind, k, e)
        seen += 1
    assert seen >= 10
    # an optimiser step on these gradients, then the next forward sees the new weights
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    opt.step()
    m.weights_changed()
    torch.manual_seed(99)
    out2 = (m(pkg.convert_to_one_hot(d, 342), c) if kind == "single" else
            m(pkg.convert_to_one_hot(d, 342), pkg.convert_to_one_hot(r, 3), pkg.convert_to_one_hot(n, 16), c, rd32, nd32))[0]
    out2 = out2[0] if kind == "fader" else out2
    assert float((out2.detach() - out.detach()).abs().max()) > 1e-6


# ---- the five model_config_v2.json trainers: epoch drivers vs the reference's own training_phase (tests/golden/epoch_v2.npz) ---------------
V2_FAMILIES = {"vae": ("MusicAttrRegVAE", "VAETrainer"), "singlevae": ("MusicAttrSingleVAE", "SingleVAETrainer"), "cvae": ("MusicAttrCVAE", "CVAETrainer"),
               "fader": ("MusicAttrFaderNets", "FaderTrainer"), "glsr": ("MusicAttrRegVAE", "GLSRTrainer")}


def make_v2_family(pkg, family, g, device="cpu", ops=None):
    """the seeded model of make_golden_epoch_v2.py for `family` (GLSR: output layer rescaled like the fixture) + its trainer"""
    P = family + "/"
    H, Z, B, T, TR = (int(x) for x in g[P + "dims"])
    torch.manual_seed(1234)
    m = getattr(pkg, V2_FAMILIES[family][0])(roll_dims=342, rhythm_dims=3, note_dims=16, chroma_dims=24, hidden_dims=H, z_dims=Z, n_step=T)
    if family == "glsr":
        with torch.no_grad():
            m.linear_out_g.weight.mul_(float(g[P + "out_scale"][0]))
            m.linear_out_g.bias.add_(torch.from_numpy(g[P + "bias_shift"]))
    if ops is not None:
        m._make_ops = lambda dev, _ops=ops: _ops
    m = m.to(device)
    m.train()
    return m, getattr(pkg, V2_FAMILIES[family][1])(m, lr=1e-3, beta=0.2)


def check_epoch_v2_run(pkg, family, g, tmp_path, device="cpu", ops=None, rtol=5e-4, atol_w=1e-3, noise=()):
    """pkg.training_phase_v2(family) on the golden loaders: same lines (text and numbers) as the reference's training_phase printed, same
    checkpoint key set, weights within atol_w of the saved ones, one time-stamped copy"""
    import re
    P = family + "/"
    m, tr = make_v2_family(pkg, family, g, device, ops)
    dl = lambda name, n: [tuple(torch.from_numpy(np.asarray(g[P + "%s%d_%d" % (name, i, j)])) for j in range(6)) for i in range(n)]
    lines = []
    save_path = os.path.join(str(tmp_path), "golden_%s.pt" % family)
    torch.manual_seed(4242)
    start = int(g[P + "start_step"])
    step = pkg.training_phase_v2(family, tr, start, 2, dl("tr", 2), dl("va", 1), save_path, name="golden_" + family, log=lines.append)
    assert step == start + 4
    ref = [str(l) for l in g[P + "lines"]]
    assert len(lines) == len(ref), (lines, ref)
    num = re.compile(r"-?\d+\.\d+")
    for got, want in zip(lines[:-1], ref[:-1]):
        assert num.sub("#", got) == num.sub("#", want), (got, want)
        a, b = [float(x) for x in num.findall(got)], [float(x) for x in num.findall(want)]
        np.testing.assert_allclose(a, b, rtol=rtol, atol=2e-4, err_msg=want)
    assert lines[-1].startswith("Model saved as ") and ref[-1].startswith("Model saved as ")
    saved = torch.load(save_path)
    want_keys = [k[len(P + "wend/"):] for k in g.keys() if k.startswith(P + "wend/")]
    assert sorted(saved.keys()) == sorted(want_keys)
    assert all(v.device.type == "cpu" for v in saved.values())
    for k, v in saved.items():
        if k not in noise:
            np.testing.assert_allclose(v.numpy(), g[P + "wend/" + k], rtol=0, atol=atol_w, err_msg=k)
    stamped = [f for f in os.listdir(str(tmp_path)) if f.startswith("golden_%s_" % family) and f.endswith(".pt")]
    assert len(stamped) == int(g[P + "stamped"]) == 1
    return m


# ---- GRU scans: every step of every output against an fp64 scan + autograd (tests/test_scan_reference.py, test_gpu_parity.py) ---------------
# A *logical scan* is a dict of CPU fp32 tensors that states one whole scan of fn_gru_seq_fwd / fn_gru_seq_bwd (include/fadernets.h), unchunked:
#   B, T, H, w_hh [3H][H], b_hh [3H], optional b_ih [3H], h0 [B][H], gx_dense [T][B][3H], gx_table [V][3H] + idx [B][>=T] int32 (+ reverse,
#   idx_shift, start_token), gx_rowbias [B][3H]; for the backward optional dh_last [B][H], dh_ext [T][B][H] and the flags want_dh0, want_rowsums.
#   gates=False: a forward-only scan, as every caller with save=False launches it - the descriptor gets gates = NULL, no backward runs, and
#   h_all is the one output (the ping-pong and bf16 x 6 forward kernels need saved gates: such a launch takes other kernels, csrc/gru_plan.h).
# run_scans() turns a list of them into the descriptors of a backend (FakeOps on a row subset, HipOps on the device), in one launch or in time
# chunks with the hand-overs the decoder pipeline uses, and returns per scan the outputs named in SCAN_QUANTITIES on the CPU.
# factor of check_scan_vs_f64 = the smallest power of two >= 2 x the worst err_kernel / e_ref measured on an MI355X (profiles/scan_fp64_errors.txt),
# at most SCAN_F_CAP.  Measured worst: 4.6 forward, 7.7 dh0, 1.7 row sums -> 16; dgx_all / dghn_all 13.2 would ask for 32: capped, the headroom
# there is 1.2 x
SCAN_F = 16
SCAN_F_CAP = 16            # the margin replay_decode_check already uses
SCAN_EPS = 2.0 ** -23
SCAN_MIN_REF = 2.0 ** -100           # input condition: every per-step block maximum of the fp64 reference is at least this
SCAN_BLOCK = 32            # 32 consecutive checked rows form one block of the per-step metric: every row of a scan of <= 64 rows, else (two rows per
                           # 16-row tile) the checked rows of 256 rows of the batch
SCAN_FWD_QUANTITIES = ("h_all", "gate_r", "gate_z", "gate_n", "gate_hn")
SCAN_BWD_QUANTITIES = ("dgx_all", "dghn_all", "dh0", "dgx_rowsum", "dghn_rowsum")
SCAN_QUANTITIES = SCAN_FWD_QUANTITIES + SCAN_BWD_QUANTITIES


def scan_rows(B, seed=0):
    """the rows of a B-row scan that get referenced: all of them when B <= 64, else of every 16-row tile its first row and one more row
    drawn with a fixed seed - no 16-row patch of any step or column is without two checked rows"""
    if B <= 64:
        return np.arange(B)
    rng = np.random.RandomState(seed)
    rows = []
    for r0 in range(0, B, 16):
        n = min(16, B - r0)
        rows.append(r0)
        if n > 1:
            rows.append(r0 + 1 + int(rng.randint(n - 1)))
    return np.asarray(rows, dtype=np.int64)


def _scan_tok(s, p, rows):
    tau = (s["T"] - 1 - p if s.get("reverse", 0) else p) + s.get("idx_shift", 0)
    if tau < 0:
        return torch.full((len(rows),), int(s.get("start_token", 0)), dtype=torch.long)
    return s["idx"][rows, tau].long()


def scan_reference_f64(scans, rows=None, device="cpu"):
    """float64 restatement of fn_gru_seq_fwd on rows[i] of logical scan i (rows of a scan do not interact), and its backward by torch
    autograd of   sum_p <dh_ext[p], h_p> + <dh_last, h_{T-1}>   through that forward: dgx_all = d/d(input-side gate pre-activations) (the leaf
    gx_dense, or a zero probe added to them), dghn_all = d/d(zero probe added to W_hn h + b_hn), dh0 = d/d(h0), the row sums = their sums over
    time.  Chunked launches are referenced as the one scan they are equivalent to.  device: where plain torch evaluates it (float64 on the GPU is as
    independent of the HIP kernels as on the CPU, and much faster at the 256-step shapes).  Returns per scan {quantity: float64 CPU tensor}."""
    out = []
    for i, s in enumerate(scans):
        rw = torch.as_tensor(np.arange(s["B"]) if rows is None else rows[i], dtype=torch.long)
        R, T, H = len(rw), s["T"], s["H"]
        f = lambda k: None if s.get(k) is None else s[k].to(device).double()
        W, b_hh, b_ih, tab = f("w_hh"), f("b_hh"), f("b_ih"), f("gx_table")
        rb = None if s.get("gx_rowbias") is None else s["gx_rowbias"][rw].to(device).double()
        backward = (s.get("dh_last") is not None or s.get("dh_ext") is not None) and s.get("gates", True)
        with torch.enable_grad():
            pgx = (s["gx_dense"][:, rw].to(device).double() if s.get("gx_dense") is not None else torch.zeros(T, R, 3 * H, dtype=torch.float64, device=device)).requires_grad_(backward)
            phn = torch.zeros(T, R, H, dtype=torch.float64, device=device, requires_grad=backward)
            h0 = (s["h0"][rw].to(device).double() if s.get("h0") is not None else torch.zeros(R, H, dtype=torch.float64, device=device)).requires_grad_(backward)
            h, hs, gs = h0, [], []
            for p in range(T):
                gx = pgx[p]
                if b_ih is not None:
                    gx = gx + b_ih
                if tab is not None:
                    gx = gx + tab[_scan_tok(s, p, rw).to(device)]
                if rb is not None:
                    gx = gx + rb
                gh = h @ W.t() + b_hh
                hn = gh[:, 2 * H:] + phn[p]
                r = torch.sigmoid(gx[:, :H] + gh[:, :H])
                z = torch.sigmoid(gx[:, H:2 * H] + gh[:, H:2 * H])
                n = torch.tanh(gx[:, 2 * H:] + r * hn)
                h = (1 - z) * n + z * h
                hs.append(h)
                gs.append((r.detach(), z.detach(), n.detach(), hn.detach()))
            o = {"h_all": torch.stack([x.detach() for x in hs])}
            for j, k in enumerate(SCAN_FWD_QUANTITIES[1:] if s.get("gates", True) else ()):
                o[k] = torch.stack([g_[j] for g_ in gs])
            if backward:
                loss = torch.zeros((), dtype=torch.float64, device=device)
                if s.get("dh_last") is not None:
                    loss = loss + (s["dh_last"][rw].to(device).double() * hs[-1]).sum()
                if s.get("dh_ext") is not None:
                    loss = loss + (s["dh_ext"][:, rw].to(device).double() * torch.stack(hs)).sum()
                o["dgx_all"], o["dghn_all"], dh0 = torch.autograd.grad(loss, [pgx, phn, h0])
                if s.get("want_dh0"):
                    o["dh0"] = dh0
                if s.get("want_rowsums", True):
                    o["dgx_rowsum"], o["dghn_rowsum"] = o["dgx_all"].sum(0), o["dghn_all"].sum(0)
        out.append({k: v.detach().cpu() for k, v in o.items()})
    return out


def _unblock_gates(g, B, H, rows=None):
    """the HIP kernels' private gate layout (gate_off in csrc/gru.hip) -> [T][B][4][H] (rows given: [T][len(rows)][4][H], those rows only)"""
    T = g.shape[0]
    nrt = (B + 15) // 16
    b = (torch.arange(B) if rows is None else torch.as_tensor(rows, dtype=torch.long)).view(-1, 1, 1)
    q = torch.arange(4).view(1, 4, 1)
    u = torch.arange(H).view(1, 1, H)
    off = ((((u // 16) * nrt + (b // 16)) * 4 + q) * 4 + (b % 4)) * 64 + ((b % 16) // 4) * 16 + (u % 16)
    return g[:, off.reshape(-1).to(g.device)].view(T, b.shape[0], 4, H)


def run_scans(ops, scans, rows=None, device="cpu", chunk=None, x6=False, fwd_kw=None, bwd_kw=None, carry_fault=None, h_all_off=0):
    """The logical scans through a backend: ops = FakeOps (device "cpu", restricted to rows[i] of scan i) or HipOps (all rows on `device`; the
    outputs are cut to rows[i] afterwards).  chunk = None: one forward and one backward launch.  chunk = CH: time chunks of CH steps, the forward
    state handed from launch to launch as operand images (h_last_frag -> h0_frag), the backward state gradient through dh0 -> dh_last with time
    running backwards over the chunks - what the decoder pipeline does (engine.py, _bwd_chunk).  x6: the arithmetic asked for, explicitly
    (HipOps: dw_x6 and x6= of both calls; a launch that cannot take it raises).  carry_fault(ci, tensor): test hook, edits the CPU carry that
    leaves backward chunk ci (FakeOps only).  h_all_off: h_all is a view that many floats behind the start of its allocation (1: 4 bytes off a
    16-byte boundary).  The backward consumes the backend's OWN saved gates.  A scan with gates=False is handed gates = None and gets no backward:
    its one output is h_all.  Returns per scan {quantity: CPU tensor}."""
    fake = device == "cpu"
    fwd_kw, bwd_kw = dict(fwd_kw or {}), dict(bwd_kw or {})
    if not fake:
        fwd_kw["x6"], bwd_kw["x6"] = x6, x6
    rws = [torch.as_tensor(np.arange(s["B"]) if rows is None else rows[i], dtype=torch.long) for i, s in enumerate(scans)]
    dev = lambda t: t.to(device).contiguous()
    zeros = lambda *shape: torch.zeros(*shape, device=device)
    fw, bw, sub = [], [], []
    for s, rw in zip(scans, rws):
        take = (lambda t, dim=0: t.index_select(dim, rw)) if fake else (lambda t, dim=0: t)     # FakeOps runs the referenced rows only
        B, T, H = (len(rw) if fake else s["B"]), s["T"], s["H"]
        sub.append((B, T, H))
        d = dict(B=B, T=T, H=H, reverse=int(s.get("reverse", 0)), b_hh=dev(s["b_hh"]), idx_shift=int(s.get("idx_shift", 0)), start_token=int(s.get("start_token", 0)),
                 h_all=zeros(T * B * H + h_all_off)[h_all_off:].view(T, B, H), gates=zeros(T, ops.gates_floats(B, H)) if s.get("gates", True) else None)
        w = dev(s["w_hh"])
        d["w_hh_frag"] = zeros(ops.frag_floats(3 * H, H))
        b = dict(B=B, T=T, H=H, w_hh_t_frag=zeros(ops.frag_floats(H, 3 * H)))
        if fake:
            ops.frag_pack(w, d["w_hh_frag"]), ops.frag_pack(w.t().contiguous(), b["w_hh_t_frag"])
        else:
            jobs = [("frag", w, d["w_hh_frag"]), ("frag_t", w, b["w_hh_t_frag"])]
            if x6:
                d["w_hh_frag3"], b["w_hh_t_frag3"] = zeros(ops.frag_floats(3 * H, H) * 3 // 2), zeros(ops.frag_floats(H, 3 * H) * 3 // 2)
                jobs += [("frag3", w, d["w_hh_frag3"]), ("frag3_t", w, b["w_hh_t_frag3"])]
            ops.weight_images(jobs)
        for k in ("b_ih", "gx_table"):
            if s.get(k) is not None:
                d[k] = dev(s[k])
        for k in ("h0", "gx_rowbias", "idx"):
            if s.get(k) is not None:
                d[k] = dev(take(s[k]))
        if s.get("gx_dense") is not None:
            d["gx_dense"] = dev(take(s["gx_dense"], 1))
        fw.append(d)
        if (s.get("dh_last") is not None or s.get("dh_ext") is not None) and s.get("gates", True):
            b.update(h0=d.get("h0"), h_all=d["h_all"], gates=d["gates"], dh_last=None if s.get("dh_last") is None else dev(take(s["dh_last"])),
                     dh_ext=None if s.get("dh_ext") is None else dev(take(s["dh_ext"], 1)), dgx_all=zeros(T, B, 3 * H), dghn_all=zeros(T, B, H),
                     dh0=zeros(B, H) if s.get("want_dh0") else None, scratch=zeros(B, H))
            if s.get("want_rowsums", True):
                b["dgx_rowsum"], b["dghn_rowsum"] = zeros(B, 3 * H), zeros(B, H)
            bw.append(b)
        else:
            bw.append(None)
    if chunk is None:
        ops.gru_seq_fwd(fw, **fwd_kw)
    else:
        T = scans[0]["T"]
        assert all(s["T"] == T and not s.get("reverse", 0) for s in scans), "chunked chains: forward scans of one length"
        hand = [[zeros(ops.frag_floats(B, H) * (3 if x6 and not fake else 2) // 2) for _ in range(2)] for B, _, H in sub]
        for ci, t0 in enumerate(range(0, T, chunk)):
            t1 = min(T, t0 + chunk)
            part = []
            for d, hb in zip(fw, hand):
                c = dict(d, T=t1 - t0, h_all=d["h_all"][t0:t1], gates=None if d["gates"] is None else d["gates"][t0:t1], idx_shift=d["idx_shift"] + t0)
                if d.get("gx_dense") is not None:
                    c["gx_dense"] = d["gx_dense"][t0:t1]
                if t0 > 0:
                    c["h0"], c["h0_frag"] = d["h_all"][t0 - 1], hb[(ci - 1) & 1]
                if t1 < T:
                    c["h_last_frag"] = hb[ci & 1]
                part.append(c)
            ops.gru_seq_fwd(part, **fwd_kw)
    live = [b for b in bw if b is not None]
    if live and chunk is None:
        ops.gru_seq_bwd(live, **bwd_kw)
    elif live:
        assert len(live) == len(bw)
        carry = [[zeros(B, H) for _ in range(2)] for B, _, H in sub]
        starts = list(reversed(range(0, T, chunk)))
        for ci, t0 in enumerate(starts):
            t1 = min(T, t0 + chunk)
            part = []
            for b, cr in zip(bw, carry):
                c = dict(b, T=t1 - t0)
                for k in ("h_all", "gates", "dh_ext", "dgx_all", "dghn_all"):
                    if b.get(k) is not None:
                        c[k] = b[k][t0:t1]
                if t0 > 0:
                    c["h0"] = b["h_all"][t0 - 1]
                    c["dh0"] = cr[ci & 1]
                if t1 < T:
                    c["dh_last"] = cr[(ci - 1) & 1]
                part.append(c)
            ops.gru_seq_bwd(part, **bwd_kw)
            if carry_fault is not None and t0 > 0:
                for cr in carry:
                    carry_fault(ci, cr[ci & 1])
    out = []
    for s, rw, d, b, (B, T, H) in zip(scans, rws, fw, bw, sub):
        cut = (lambda t, dim=0: t.cpu()) if fake else (lambda t, dim=0: t.index_select(dim, rw.to(device)).cpu())
        o = {"h_all": cut(d["h_all"], 1)}
        if d["gates"] is not None:
            gt = d["gates"][:, : B * 4 * H].reshape(T, B, 4, H) if fake else _unblock_gates(d["gates"], B, H, rw).cpu()
            for j, k in enumerate(SCAN_FWD_QUANTITIES[1:]):
                o[k] = gt[:, :, j]
        if b is not None:
            for k in SCAN_BWD_QUANTITIES:
                if b.get(k) is not None:
                    o[k] = cut(b[k], 1 if k.endswith("_all") else 0)
        out.append(o)
    return out


def scan_step_errors(got, ref64, rows):
    """{(scan, quantity): (err, refmax)}, both [steps][blocks] float64 arrays (one step for dh0 and the row sums): for every step and every
    block of SCAN_BLOCK consecutive checked rows   err = max |got - ref64| / max |ref64|   over THAT block of THAT step, all
    columns - never over the whole tensor.  A quantity the reference has and `got` lacks is an error."""
    res = {}
    for i, (g_, r_) in enumerate(zip(got, ref64)):
        blk = np.arange(len(rows[i])) // SCAN_BLOCK
        ids = np.unique(blk)
        for k, ref in r_.items():
            assert k in g_, "scan %d: output %s missing" % (i, k)
            a, ref = g_[k].double(), ref.double()
            if a.dim() == 2:
                a, ref = a.unsqueeze(0), ref.unsqueeze(0)
            assert a.shape == ref.shape, (i, k, tuple(a.shape), tuple(ref.shape))
            err, den = np.zeros((a.shape[0], len(ids))), np.zeros((a.shape[0], len(ids)))
            for j, bid in enumerate(ids):
                m = torch.from_numpy(np.nonzero(blk == bid)[0])
                dd = (a[:, m] - ref[:, m]).abs().flatten(1)
                num = torch.where(torch.isnan(dd).any(1), torch.full((dd.shape[0],), float("nan"), dtype=torch.float64), dd.amax(1))
                den[:, j] = ref[:, m].abs().flatten(1).amax(1).numpy()
                err[:, j] = num.numpy() / den[:, j]
            res[(i, k)] = (err, den)
    return res


_SCAN_REF_CACHE = {}


def scan_references(scans, rows, chunk=None, key=None, ref_device="cpu"):
    """(fp64 reference, e_ref) of a case: e_ref = scan_step_errors of FakeOps in fp32 on the same inputs, rows and chunking - what fp32 rounding
    alone costs at every step and block.  Asserts the input condition: every per-step block maximum of the fp64 reference >= 2**-100 and every
    e_ref finite and non-zero (but for the one output that is a copy of an input: gate_hn at step 0 of a scan that starts from the zero state).  key: cache name (the cases of a test module share inputs between launch variants)."""
    if key is not None and key in _SCAN_REF_CACHE:
        return _SCAN_REF_CACHE[key]
    from fake_ops import FakeOps
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    try:
        ref64 = scan_reference_f64(scans, rows, ref_device)
        fake = run_scans(FakeOps(), scans, rows, chunk=chunk)
    finally:
        torch.set_num_threads(threads)
    e_ref = scan_step_errors(fake, ref64, rows)
    for (i, k), (e, den) in e_ref.items():
        assert den.min() >= SCAN_MIN_REF, "input condition: scan %d %s has a per-step block maximum of %.3e < 2**-100 (step %d)" % (
            i, k, den.min(), int(np.argwhere(den == den.min())[0][0]))
        ok = np.isfinite(e) & (e > 0)
        if k == "gate_hn" and scans[i].get("h0") is None:
            ok[0] = np.isfinite(e[0])        # from a zero state W_hn h + b_hn IS the input b_hn: exact in every arithmetic, e_ref = 0 (the bound is then F * 2**-23)
        assert ok.all(), "input condition: scan %d %s: e_ref is 0 or not finite at step %d" % (i, k, int(np.argwhere(~ok)[0][0]))
    if key is not None:
        _SCAN_REF_CACHE[key] = (ref64, fake, e_ref)
    return ref64, fake, e_ref


def check_scan_vs_f64(scans, got, rows, chunk=None, key=None, F=None, ref_device="cpu"):
    """Every output of a scan launch (or chain of launches) against the fp64 scan + autograd, step by step:
      (new)  err[p, block] <= F * max(e_ref[p, block], 2**-23)   for every scan, quantity, step p and row block (scan_step_errors), where e_ref is
             the fp32 CPU restatement's own distance from fp64 on the same inputs: the margin F covers another summation order and another
             draw of inputs, not a wrong term;
      (old)  the whole-tensor bound the suite already applies, unchanged: max |got - ref| <= 2e-5 (forward) / 5e-5 (backward) of the tensor's max.
    A forward-only scan (gates=False) has h_all alone, checked at every step with the same bound and factor.
    Returns {(scan, quantity): (worst err / max(e_ref, 2**-23), step, block)}."""
    F = SCAN_F if F is None else F
    assert F <= SCAN_F_CAP
    ref64, fake, e_ref = scan_references(scans, rows, chunk, key, ref_device)
    err = scan_step_errors(got, ref64, rows)
    worst, bad = {}, []
    for (i, k), (e, den) in err.items():
        ratio = e / np.maximum(e_ref[(i, k)][0], SCAN_EPS)
        flat = np.where(np.isnan(ratio), np.inf, ratio)
        p, j = np.unravel_index(int(np.argmax(flat)), flat.shape)
        worst[(i, k)] = (float(flat[p, j]), int(p), int(j))
        if not flat[p, j] <= F:
            cols = (got[i][k].double() - ref64[i][k]).abs()
            bad.append("scan %d %s: err %.3e = %.1f x e_ref %.3e at step %d, row block %d (%d of %d steps x blocks over F = %g; worst column %d)" % (
                i, k, e[p, j], flat[p, j], e_ref[(i, k)][0][p, j], p, j, int((~(flat <= F)).sum()), flat.size, F,
                int((cols[p] if cols.dim() == 3 else cols).amax(0).argmax())))
        tol = 2e-5 if k in SCAN_FWD_QUANTITIES else 5e-5
        whole = relerr(got[i][k].double().numpy(), ref64[i][k].numpy())
        if not whole < tol:
            bad.append("scan %d %s: whole-tensor rel err %.3e >= %g" % (i, k, whole, tol))
    assert not bad, "\n".join(bad)
    return worst


class PlanRecorder:
    """HipOps with every gru_seq_fwd / gru_seq_bwd preceded by the library's own plan for the same arguments (ops.gru_fwd_plan / gru_bwd_plan on the
    real descriptors, current device): .fwd / .bwd collect the plans, one per launch"""

    def __init__(self, ops):
        self.ops, self.fwd, self.bwd = ops, [], []

    def __getattr__(self, name):
        return getattr(self.ops, name)

    def gru_seq_fwd(self, scans, **kw):
        self.fwd.append(self.ops.gru_fwd_plan(scans, **kw))
        self.ops.gru_seq_fwd(scans, **kw)

    def gru_seq_bwd(self, scans, **kw):
        self.bwd.append(self.ops.gru_bwd_plan(scans, **kw))
        self.ops.gru_seq_bwd(scans, **kw)


def chosen_kernels(plans):
    """the kernel every recorded plan says its launch takes"""
    for p in plans:
        assert p["status"] == 0 and p["chosen"] is not None and p["candidates"][p["chosen"]]["fits"] is not False, p
    return [p["candidates"][p["chosen"]]["kernel"] for p in plans]


def scan_lines(case, kernels, worst):
    """the lines of profiles/scan_fp64_errors.txt for one case: per quantity the worst ratio over the scans and where it occurred"""
    out = []
    for q in SCAN_QUANTITIES:
        hits = [(v, i) for (i, k), v in worst.items() if k == q]
        if hits:
            (ratio, p, j), i = max(hits)
            out.append("%-34s %-58s %-12s ratio %6.3f  scan %d step %3d block %d" % (case, kernels[0] if q in SCAN_FWD_QUANTITIES else kernels[1], q, ratio, i, p, j))
    return out


def _logical_scan(gen, B, T, H, kind, h0=True, rowbias=False, b_ih=True, dh_last=0.0, dh_ext=0.0, want_dh0=False, want_rowsums=True, V=57):
    """one seeded logical scan; kind: "table" / "table_rev" / "table_shift" (idx_shift -1 + start_token) / "dense"; dh_last / dh_ext: the scale of
    the N(0, 1) gradient seeds, 0 = absent.  Weights randn / sqrt(H), as the kernel tests of test_gpu_parity.py draw them."""
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    s = dict(B=B, T=T, H=H, w_hh=rn(3 * H, H) / H ** 0.5, b_hh=rn(3 * H) * 0.1, want_dh0=want_dh0, want_rowsums=want_rowsums)
    if b_ih:
        s["b_ih"] = rn(3 * H) * 0.1
    if h0:
        s["h0"] = rn(B, H) * 0.5
    if rowbias:
        s["gx_rowbias"] = rn(B, 3 * H) * 0.3
    if kind == "dense":
        s["gx_dense"] = rn(T, B, 3 * H) * 0.5
    else:
        s["gx_table"] = rn(V, 3 * H) * 0.5
        s["idx"] = torch.randint(0, V, (B, T), generator=gen, dtype=torch.int32)
        s["reverse"] = int(kind == "table_rev")
        if kind == "table_shift":
            s["idx_shift"], s["start_token"] = -1, V - 1
    if dh_last:
        s["dh_last"] = rn(B, H) * dh_last
    if dh_ext:
        s["dh_ext"] = rn(T, B, H) * dh_ext
    return s


def _forward_only(scans):
    """the same logical scans as forward-only ones: no saved gates, hence no backward (a gradient seed they carry is not used)"""
    return [dict(s, gates=False) for s in scans]


def _ws_scans(gen, B, H, T=70, n=2):
    """the inputs of the 32-slice / per-step cases: a reverse table scan with h0, row bias, dh_last only and dL/dh0, beside (n = 2) a dense scan
    from a zero state with dh_ext only"""
    sc = [_logical_scan(gen, B, T, H, "table_rev", rowbias=True, dh_last=1.0, want_dh0=True)]
    if n > 1:
        sc.append(_logical_scan(gen, B, T, H, "dense", h0=False, b_ih=False, dh_ext=0.5))
    return sc


# name -> (seed, builder(gen) -> logical scans, chunk).  The shapes are the production launches of engine.py and the edges of the dispatch in
# csrc/gru_plan.h; tests/test_scan_reference.py runs every one of them on the CPU, tests/test_gpu_parity.py on the kernels.
SCAN_INPUTS = {
    # encoder: 4 scans x 256 rows x 256 steps, token tables, two reverse, gradient from the last state only.  dh_last x 2**40 (exact in fp32): with
    # w_hh = randn / sqrt(H) the gate gradients shrink by ~2**-0.47 per step, 2**-120 over the launch - the scale keeps every step's maximum
    # above 2**-100, away from the subnormal range where a flush-to-zero GPU and the CPU differ for reasons that are no bugs
    "enc": (11, lambda g: [_logical_scan(g, 256, 256, 512, k, h0=False, dh_last=2.0 ** 40) for k in ("table", "table_rev", "table", "table_rev")], None),
    # decoder pipeline: 2 scans x 256 rows x 256 steps as 8 chained launches of 32 steps (226 steps: a tail chunk of 2), dh_ext at every step
    "dec": (12, lambda g: [_logical_scan(g, 256, 256, 512, "table_shift", rowbias=True, dh_ext=0.5, want_dh0=True),
                           _logical_scan(g, 256, 256, 512, "dense", b_ih=False, dh_ext=0.5, want_dh0=True)], 32),
    "dec_tail": (13, lambda g: [_logical_scan(g, 256, 226, 512, "table_shift", rowbias=True, dh_ext=0.5, want_dh0=True),
                                _logical_scan(g, 256, 226, 512, "dense", b_ih=False, dh_ext=0.5, want_dh0=True)], 32),
    # attribute sub-decoders: 2 scans x 256 rows x 64 steps, h0 given, dh_ext every step, dL/dh0 wanted
    "attr": (14, lambda g: [_logical_scan(g, 256, 64, 512, "table", rowbias=True, dh_ext=0.5, want_dh0=True) for _ in range(2)], None),
    "ws_256x2": (15, lambda g: _ws_scans(g, 256, 512), None),
    "ws_256x4": (16, lambda g: _ws_scans(g, 256, 512) + _ws_scans(g, 256, 512), None),
    "t2": (17, lambda g: _ws_scans(g, 256, 512, T=2), None),
    "t1": (18, lambda g: _ws_scans(g, 256, 512, T=1), None),
    # 8 scans of different lengths in one call: every input kind, h0 beside none, a scan without dh_last beside one without dh_ext
    "eight": (19, lambda g: [_logical_scan(g, 64, 3 + 2 * i, 512, ("table", "table_rev", "table_shift", "dense")[i % 4], h0=bool(i & 1), rowbias=i % 3 == 0,
                                           dh_last=float(i % 3 != 1), dh_ext=0.5 * (i % 3 != 0), want_dh0=bool(i & 1), want_rowsums=i != 5) for i in range(8)], None),
}
for _B in (1, 33, 200):
    for _H in (64, 96, 512):
        SCAN_INPUTS["ws_%d_%d" % (_B, _H)] = (100 + _B + _H, (lambda g, B=_B, H=_H: _ws_scans(g, B, H, n=1 if (B, H) == (200, 512) else 2)), None)
# forward only (gates = NULL): what save=False launches.  Small: each case takes seconds.
SCAN_INPUTS.update({
    # the encoder launch of Engine.encode(save=False): 4 scans x 256 rows, two reversed -> 128-row groups, no ping-pong without gates
    "fo_enc": (31, lambda g: _forward_only([_logical_scan(g, 256, 6, 512, k, h0=False) for k in ("table", "table_rev", "table", "table_rev")]), None),
    # the decoder pipeline's two layers, 7 steps in chunks of 2: fp32 fragment hand-over through both slots, a one-step tail on the per-step kernel
    "fo_dec": (32, lambda g: _forward_only([_logical_scan(g, 256, 7, 512, "table_shift", rowbias=True), _logical_scan(g, 256, 7, 512, "dense", b_ih=False)]), 2),
    "fo_33_96": (33, lambda g: _forward_only(_ws_scans(g, 33, 96, T=9)), None),
    "fo_200_64": (34, lambda g: _forward_only(_ws_scans(g, 200, 64, T=9)), None),
    "fo_step": (35, lambda g: _forward_only(_ws_scans(g, 33, 512, T=5)), None),
})
_SCAN_INPUT_CACHE = {}


def scan_inputs(name):
    """(logical scans, checked rows per scan, chunk) of a named case, built once"""
    if name not in _SCAN_INPUT_CACHE:
        seed, build, chunk = SCAN_INPUTS[name]
        scans = build(torch.Generator().manual_seed(seed))
        _SCAN_INPUT_CACHE[name] = (scans, [scan_rows(s["B"], seed + i) for i, s in enumerate(scans)], chunk)
    return _SCAN_INPUT_CACHE[name]


# FnGruFwd / FnGruBwd .variant bits (music-fader-nets_amd/_lib.py; repeated here so that the CPU tests need no library)
_V_ROWS, _V_ALT, _V_LOOPS, _V_NOPP, _V_NORS, _V_X6ALT = 0xFF, 0x100, 0x400, 0x800, 0x2000, 0x8000


def scan_kernel_candidates(scans, variants=(0, 0), x6=False, cu_budget=(0, 0), persistent=True, T=None, cus=256, aligned=(True, True)):
    """(forward, backward) kernel instances a launch of these scans can take, in the order the launch tries them: the dispatch of csrc/gru_plan.h
    restated on shapes, independently of it (tests/test_scan_reference.py compares the two).  The launch takes the first candidate whose workgroups
    are all resident at once - which only the device can say, so where that can change the outcome the whole list is given; the per-step kernel needs
    no residency and is last.  A bf16 x 6 launch has one candidate, or none (the call is refused).  T: the steps per launch of a chunked chain;
    variants, cu_budget: (forward, backward); aligned: are the operands of the 16-byte epilogue vectors 16-byte aligned (else: per step);
    a scan with gates=False saves no gates."""
    H = scans[0]["H"]
    Bs = [s["B"] for s in scans]
    Ts = [s["T"] if T is None else T for s in scans]
    one_src = all((s.get("gx_table") is not None) != (s.get("gx_dense") is not None) for s in scans)
    gates = all(s.get("gates", True) for s in scans)
    ceil = lambda a, b: (a + b - 1) // b
    names = []
    for back in (False, True):
        variant = variants[back]
        step = "gru_bwd_step_kernel" if back else "gru_fwd_step_kernel"
        budget = cu_budget[back]
        c = budget if 0 < budget < cus else cus
        nsl = H // 16
        if not persistent or H > 512 or any(s["H"] != H for s in scans) or not aligned[back] or max(Ts) < 2 or nsl > c:
            names.append([] if x6 else [step])
            continue
        maxgroups = min(c // nsl, 64)

        def pick_rows():
            for rpw in (16, 32, 64, 128):
                if variant & _V_ROWS in (0, rpw) and sum(ceil(B, rpw) for B in Bs) <= maxgroups:
                    return rpw
            return 0
        ksplit = lambda rpw: 4 if rpw == 16 else 2 if rpw == 32 else 2 if (rpw == 64 and not variant & _V_ALT) else 1
        full = lambda r: all(B % r == 0 for B in Bs)
        if not back:
            if x6:
                ok = H == 512 and min(Ts) >= 2 and gates
                mt = 1 if ok and full(64) and sum(Bs) // 64 <= min(c // 32, 64) else 2 if ok and full(128) and sum(Bs) // 128 <= min(c // 32, 64) else 0
                pp = not variant & _V_X6ALT and mt and 2 * sum(Bs) // (64 * mt) <= 64 and one_src
                names.append([] if not mt else ["gru_fwd_x6pp_kernel<%d>" % (3 - mt) if pp else "gru_fwd_x6_kernel<%d>" % mt])
                continue
            rpw = pick_rows()
            if not rpw:
                names.append([step])
                continue
            wk = ksplit(rpw)
            pp = H == 512 and (rpw == 128 or (rpw == 64 and wk == 2)) and not variant & (_V_LOOPS | _V_NOPP) and 2 * sum(ceil(B, rpw) for B in Bs) <= 64 \
                and full(rpw) and min(Ts) >= 2 and one_src and gates
            tiling = {128: "4, 1, 2", 64: "4, 1, 1" if variant & _V_ALT else "2, 2, 2", 32: "2, 2, 1", 16: "1, 4, 1"}[rpw]
            names.append(["gru_fwd_pp_kernel<%d>" % (1 if rpw == 128 else 2) if pp else "gru_fwd_persist_kernel<%s, 4>" % tiling, step])
            continue

        def rs_tiles(half_chip_ok, rows32_ok):
            if H != 512 or min(Ts) < 2:
                return 0
            g64, g32 = sum(Bs) // 64, sum(Bs) // 32
            if full(64) and (g64 > 8 or (half_chip_ok and g64 * 16 == c)) and g64 <= 16 and g64 * 16 <= c:
                return 2
            return 1 if rows32_ok and full(32) and g32 > 8 and g32 <= 16 and g32 * 16 <= c else 0
        if x6:
            th = rs_tiles(True, bool(variant & _V_X6ALT))
            names.append(["gru_bwd_x6_kernel<%d>" % th] if th else [])
            continue
        th = 0 if variant & (_V_LOOPS | _V_NOPP | _V_NORS | _V_ROWS) else rs_tiles(False, True)
        rpw = pick_rows()
        tiling = {128: "4, 1, 2", 64: "4, 1, 1" if variant & _V_ALT else "2, 2, 2", 32: "2, 2, 1", 16: "1, 4, 1", 0: ""}[rpw]
        names.append((["gru_bwd_rs_kernel<%d>" % th] if th else []) + (["gru_bwd_persist_kernel<%s, 8>" % tiling] if rpw else []) + [step])
    return tuple(names)


def scan_kernel_names(scans, variants=(0, 0), x6=False, cu_budget=(0, 0), persistent=True, T=None, cus=256, aligned=(True, True)):
    """(forward, backward) kernel instance a launch of these scans takes when the device keeps every candidate resident: the first of
    scan_kernel_candidates, for the labels of profiles/scan_fp64_errors.txt and so that a case can assert that its shape reaches the kernel it is
    meant for (the GPU test asks the library which candidate the device took)."""
    cands = scan_kernel_candidates(scans, variants, x6, cu_budget, persistent, T, cus, aligned)
    assert all(cands), "not eligible for the bf16 x 6 %s" % ("backward" if cands[0] else "forward")
    return tuple(c[0] for c in cands)


def lib_scan_candidates(scans, variants=(0, 0), x6=False, cu_budget=(0, 0), persistent=True, T=None, cus=256, aligned=(True, True)):
    """what the library plans for the launch scan_kernel_candidates describes (fn_gru_fwd_plan / fn_gru_bwd_plan with the compute units given: pure
    host functions, no device): (forward, backward) candidate names in order, [] for a refused bf16 x 6 call.  The descriptors carry made-up
    addresses - the plan looks at NULL-ness and alignment only -: 16-byte aligned ones, h_all (forward) / dgx_all (backward) 4 bytes off when not
    `aligned`."""
    import ctypes
    from mfn_import import load_package
    load_package()
    from music_fader_nets_amd import _lib
    lib, n = _lib.load(), len(scans)
    A, out = 0x10000, []
    opt = lambda s, k: A if s.get(k) is not None else None
    for back in (False, True):
        arr = ((_lib.FnGruBwd if back else _lib.FnGruFwd) * n)()
        for d, s in zip(arr, scans):
            d.B, d.T, d.H = s["B"], s["T"] if T is None else T, s["H"]
            d.frag_ws, d.h0, d.cu_budget = A, opt(s, "h0"), cu_budget[back]
            d.sync_ws = A if persistent else None
            d.variant = variants[back] | (_lib.GRU_BF16X6 if x6 else 0)
            d.h_all = A if back or aligned[0] else A + 4
            d.gates = A if back or s.get("gates", True) else None       # (saved gates are optional in the forward call only)
            if back:
                d.w_hh_t_frag = d.dghn_all = d.scratch = A
                d.dgx_all = A if aligned[1] else A + 4
                d.dh_last, d.dh_ext, d.dh0 = opt(s, "dh_last"), opt(s, "dh_ext"), A if s.get("want_dh0") else None
            else:
                d.w_hh_frag = d.b_hh = A
                d.b_ih, d.gx_dense, d.gx_table, d.gx_rowbias = opt(s, "b_ih"), opt(s, "gx_dense"), opt(s, "gx_table"), opt(s, "gx_rowbias")
                d.idx, d.idx_ld = A, 1
        plan = _lib.FnGruPlan()
        rc = (lib.fn_gru_bwd_plan if back else lib.fn_gru_fwd_plan)(arr, n, cus, ctypes.byref(plan))
        assert rc == 0 and plan.status in (0, _lib.FN_E_UNSUPPORTED), (rc, plan.status)
        p = plan.as_dict()
        assert (plan.status == 0) == bool(p["candidates"]) and all(c["fits"] is None for c in p["candidates"] if c["resident"])
        out.append([c["kernel"] for c in p["candidates"]])
    return tuple(out)


# The GPU cases of test_gpu_parity.test_scans_every_step_vs_fp64: (case id, inputs, both arithmetics?, launch keywords, kernels the case is for).
# A case whose shape does not reach the kernels named here fails (scan_kernel_names, and on the GPU the library's own plan).
def _sc(cid, inputs, fwd, bwd, x6=False, variant=0, bvariant=None, budget=0, persistent=True):
    """variant: of the forward and (bvariant None) the backward launches; budget: cu_budget of the backward launches, as engine.py gives the decoder
    pipeline's backward half of the chip.  fwd / bwd: the kernel the case is for (None: any), or {steps per launch: kernel} where the launches of a
    chunked chain take different ones; a forward-only case (inputs with gates=False) runs no backward and names none."""
    return dict(id=cid, inputs=inputs, x6=x6, variants=(variant, variant if bvariant is None else bvariant), budget=(0, budget), persistent=persistent,
                kernels=(fwd, bwd))


def case_kernel(case, i, T=None):
    """the forward (i = 0) / backward (i = 1) kernel a case is for, at T steps per launch"""
    want = case["kernels"][i]
    return want.get(T) if isinstance(want, dict) else want


def case_forward_only(case):
    return not all(s.get("gates", True) for s in scan_inputs(case["inputs"])[0])


_P4, _P8 = "gru_fwd_persist_kernel<%s, 4>", "gru_bwd_persist_kernel<%s, 8>"
SCAN_CASES = [
    _sc("enc-f32", "enc", "gru_fwd_pp_kernel<1>", "gru_bwd_rs_kernel<2>"),
    _sc("enc-x6", "enc", "gru_fwd_x6pp_kernel<1>", "gru_bwd_x6_kernel<2>", x6=True),
    _sc("dec-f32", "dec", "gru_fwd_pp_kernel<2>", "gru_bwd_rs_kernel<1>"),
    _sc("dec-f32-half", "dec", "gru_fwd_pp_kernel<2>", _P8 % "4, 1, 2", budget=128),
    _sc("dec-x6-32rows", "dec", "gru_fwd_x6pp_kernel<2>", "gru_bwd_x6_kernel<1>", x6=True, bvariant=_V_X6ALT),
    _sc("dec-x6-half", "dec", "gru_fwd_x6pp_kernel<2>", "gru_bwd_x6_kernel<2>", x6=True, budget=128),
    _sc("dec_tail-f32", "dec_tail", "gru_fwd_pp_kernel<2>", "gru_bwd_rs_kernel<1>"),
    _sc("dec_tail-x6-32rows", "dec_tail", "gru_fwd_x6pp_kernel<2>", "gru_bwd_x6_kernel<1>", x6=True, bvariant=_V_X6ALT),
    _sc("dec_tail-x6-half", "dec_tail", "gru_fwd_x6pp_kernel<2>", "gru_bwd_x6_kernel<2>", x6=True, budget=128),
    _sc("attr-f32", "attr", "gru_fwd_pp_kernel<2>", "gru_bwd_rs_kernel<1>"),
    _sc("attr-x6-32rows", "attr", "gru_fwd_x6pp_kernel<2>", "gru_bwd_x6_kernel<1>", x6=True, bvariant=_V_X6ALT),
    # the 32-slice weight-stationary kernels: every forced row block and every switch, T = 70
    _sc("ws-256x2-rows64", "ws_256x2", "gru_fwd_pp_kernel<2>", _P8 % "2, 2, 2", variant=64),
    _sc("ws-256x2-rows64-alt", "ws_256x2", _P4 % "4, 1, 1", _P8 % "4, 1, 1", variant=64 | _V_ALT),
    _sc("ws-256x2-rows128", "ws_256x2", "gru_fwd_pp_kernel<1>", _P8 % "4, 1, 2", variant=128),
    _sc("ws-256x2-compiler-loops", "ws_256x2", _P4 % "2, 2, 2", _P8 % "2, 2, 2", variant=_V_LOOPS),
    _sc("ws-256x2-no-pingpong", "ws_256x2", _P4 % "2, 2, 2", _P8 % "2, 2, 2", variant=_V_NOPP),
    _sc("ws-256x2-no-rs-bwd", "ws_256x2", "gru_fwd_pp_kernel<2>", _P8 % "2, 2, 2", variant=_V_NORS),
    _sc("ws-256x2-x6-single-group", "ws_256x2", "gru_fwd_x6_kernel<1>", "gru_bwd_x6_kernel<1>", x6=True, variant=_V_X6ALT),
    _sc("ws-256x4-no-pingpong", "ws_256x4", _P4 % "4, 1, 2", _P8 % "4, 1, 2", variant=_V_NOPP),
    _sc("ws-256x4-x6-single-group", "ws_256x4", "gru_fwd_x6_kernel<2>", "gru_bwd_x6_kernel<2>", x6=True, variant=_V_X6ALT),
]
for _B, _H, _rows in ((33, 64, (16, 32, 64, 128)), (200, 64, (16, 32, 64, 128)), (33, 96, (16, 32, 64, 128)), (200, 96, (16, 32, 64, 128)),
                      (33, 512, (16, 32, 64, 128)), (200, 512, (32, 64, 128))):      # (1 x 200 rows in 16-row groups: 13 groups > the 8 that fit at H = 512)
    _til = {16: "1, 4, 1", 32: "2, 2, 1", 64: "2, 2, 2", 128: "4, 1, 2"}
    for _r in _rows:
        SCAN_CASES.append(_sc("ws-%d-%d-rows%d" % (_B, _H, _r), "ws_%d_%d" % (_B, _H), _P4 % _til[_r], _P8 % _til[_r], variant=_r))
    SCAN_CASES.append(_sc("ws-%d-%d-rows64-alt" % (_B, _H), "ws_%d_%d" % (_B, _H), _P4 % "4, 1, 1", _P8 % "4, 1, 1", variant=64 | _V_ALT))
    SCAN_CASES.append(_sc("ws-%d-%d-compiler-loops" % (_B, _H), "ws_%d_%d" % (_B, _H), None, None, variant=_V_LOOPS))
SCAN_CASES += [_sc("step-%d-%d" % (_B, _H), "ws_%d_%d" % (_B, _H), "gru_fwd_step_kernel", "gru_bwd_step_kernel", persistent=False)
               for _B in (1, 33, 200) for _H in (64, 96, 512)]
SCAN_CASES += [
    _sc("t2-f32", "t2", "gru_fwd_pp_kernel<2>", "gru_bwd_rs_kernel<1>"),
    _sc("t2-x6-32rows", "t2", "gru_fwd_x6pp_kernel<2>", "gru_bwd_x6_kernel<1>", x6=True, bvariant=_V_X6ALT),
    _sc("t1-falls-back", "t1", "gru_fwd_step_kernel", "gru_bwd_step_kernel"),
    _sc("eight-f32", "eight", "gru_fwd_pp_kernel<2>", "gru_bwd_rs_kernel<1>"),
    _sc("eight-x6-32rows", "eight", "gru_fwd_x6pp_kernel<2>", "gru_bwd_x6_kernel<1>", x6=True, bvariant=_V_X6ALT),
]
# forward only: gates = NULL reaches the weight-stationary kernels without ping-pong (all five tilings) and the per-step kernel, never pp / bf16 x 6
SCAN_CASES += [
    _sc("fo-enc", "fo_enc", _P4 % "4, 1, 2", None),
    _sc("fo-dec", "fo_dec", {2: _P4 % "2, 2, 2", 1: "gru_fwd_step_kernel"}, None),
    _sc("fo-33-96-rows16", "fo_33_96", _P4 % "1, 4, 1", None, variant=16),
    _sc("fo-33-96-rows32", "fo_33_96", _P4 % "2, 2, 1", None, variant=32),
    _sc("fo-200-64-rows16", "fo_200_64", _P4 % "1, 4, 1", None, variant=16),
    _sc("fo-200-64-rows32", "fo_200_64", _P4 % "2, 2, 1", None, variant=32),
    _sc("fo-200-64-rows64-alt", "fo_200_64", _P4 % "4, 1, 1", None, variant=64 | _V_ALT),
    _sc("fo-step", "fo_step", "gru_fwd_step_kernel", None, persistent=False),
]
