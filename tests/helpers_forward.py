"""The forward-only paths (save=False: no saved gates) and the assembled forward's outputs against the float64 oracle, per step and 16 x 32 block.

Every caller that does not train runs the model with save=False, which hands gates=None to every fn_gru_seq_fwd descriptor: the ping-pong and the
bf16 x 6 forward kernels need saved gates (csrc/gru_plan.h), so such a launch falls to gru_fwd_persist_kernel<...> or gru_fwd_step_kernel, a pipeline
asked for bf16x6 runs on fp32, and the hand-over slots hold fp32 fragments.  None of these kernels runs in the training step at the benchmark shape,
so the gradient checks of helpers_step.py say nothing about them, and the forward's outputs were compared elementwise at rtol = atol = 1e-4 only.
check_forward_outputs() states the bound of helpers_step.check_step_grads for every forward output:

    m = max |o64|,  e_ref = max |o32 - o64|,  e = max |got - o64|  over the block,      e <= FORWARD_F * max(e_ref, 2**-24 * m)

with o64 / o32 = oracle.gmvae_oracle.forward in float64 / float32 on the same weights, batch and eps.  A per-step tensor is blocked per step, as
(step, 16 batch rows, 32 columns): a stale chunk, a wrong hand-over slot or a neighbour's row group lands in blocks of its own.  A block that is
exactly zero in float64 must be exactly zero.  y_r / y_n must be the float64 argmax in every row; the references assert that every row's float64 gap
between the two largest ll is at least 2 * FORWARD_F times that row's block denominator of ll, so no row is left out.
FORWARD_F is one power of two for every case and path: at least twice the worst ratio the CPU stand-in (tests/fake_ops.py) reaches, capped at 32
(test_forward_reference.py asserts the rule; profiles/forward_fp64_errors.txt records the figures).  Nothing measured on a GPU enters it.
"""
import os
import re

import numpy as np
import torch

from helpers import lib_scan_candidates
from helpers_step import STEP_EPS, STEP_MIN_REF, block_absmax, cpu_state, gmvae_trainer, kernel_family
from oracle import gmvae_oracle as orc

FORWARD_F_CAP = 32
# the smallest power of two >= 2 x the worst FakeOps ratio over every case, path and quantity of FORWARD_PATHS: worst 4.59 (gx2 of case f, an engine
# buffer; the model's outputs alone: 3.65, qy_n of case g, which would give 8)
FORWARD_F = 16
E_VOCAB, LOGIT_LD = 342, 352

MODEL_OUTPUTS = ("out", "r_out", "n_out", "mu_r", "sigma_r", "mu_n", "sigma_n", "z_r", "z_n", "ll_r", "ll_n", "qy_r", "qy_n")
Y_OUTPUTS = ("y_r", "y_n")
ENC_BUFFERS = ("pre_r", "pre_n", "enc_h_r", "enc_h_r_reverse", "enc_h_n", "enc_h_n_reverse")
DEC_BUFFERS = ("h0g", "rbg", "hx0", "gx2", "hx1", "logits", "logits_pad")
SD_BUFFERS = ("sd_h0_r", "sd_h0_n", "sd_h_r", "sd_h_n", "sd_logits_r", "sd_logits_n")
ENGINE_BUFFERS = ENC_BUFFERS + DEC_BUFFERS + SD_BUFFERS

# path -> (cases, what it enters).  Both arithmetics run where the case lists them; the saved path of case g is the one that takes bf16 x 6 kernels.
FORWARD_PATHS = {
    "engine": ("abcdefghi", "Engine.forward(save=False, head=True), labels where the case is supervised"),
    "saved": ("adgh", "Engine.forward(save=True, head=True)"),
    "dropin": ("abceg", "model(...) in train mode under no_grad: _forward_only"),
    "encode": ("bg", "model.encode(x) under no_grad"),
    "decoder": ("ag", "model.global_decoder(z, T - 1) in train mode under no_grad"),
    "attr": ("ag", "model.sub_decoders(...) under no_grad"),
}
FORWARD_ONLY = ("engine", "dropin", "encode", "decoder", "attr")          # every launch of these paths has gates = None
PATH_NAMES = {"engine": MODEL_OUTPUTS + Y_OUTPUTS + ENGINE_BUFFERS, "saved": MODEL_OUTPUTS + Y_OUTPUTS + ENGINE_BUFFERS,
              "dropin": MODEL_OUTPUTS + Y_OUTPUTS + ENGINE_BUFFERS, "encode": ("mu_r", "sigma_r", "mu_n", "sigma_n") + ENC_BUFFERS,
              "decoder": ("out",) + DEC_BUFFERS, "attr": ("r_out", "n_out") + SD_BUFFERS}


def forward_runs(ariths=True):
    """[(path, case id, arithmetic)] of the table above: the engine paths in every arithmetic the case lists, the model's own entries in f32;
    ariths=False: one run per path and case (the CPU stand-in has one arithmetic)"""
    from helpers_step import gmvae_case
    if not ariths:
        return [(p, cid, "f32") for p, (cids, _) in FORWARD_PATHS.items() for cid in cids]
    return [(p, cid, a) for p, (cids, _) in FORWARD_PATHS.items() for cid in cids for a in (gmvae_case(cid)["ariths"] if p in ("engine", "saved") else ("f32",))]


# ---- blocks ------------------------------------------------------------------------------------------------------------------------------
def step_blocks(a):
    """[steps][row blocks][column blocks] maxima of |a| over 16 x 32 blocks of every step ([B][C]: one step)"""
    a = np.asarray(a, np.float64)
    if a.ndim == 2:
        a = a[None]
    assert a.ndim == 3, a.shape
    return np.stack([block_absmax(x) for x in a])


# ---- references --------------------------------------------------------------------------------------------------------------------------
_FWD_REF_CACHE = {}


def _tm(x):
    return x.transpose(0, 1)


def forward_references(key, build):
    """dict(o64, o32, m, e_ref, den, floor, y) of one case, cached by `key`.  build(dtype) -> {name: tensor}, per-step tensors [steps][B][C], runs
    the oracle with torch's default dtype switched to `dtype`; integer tensors (y_r, y_n) are taken from the float64 run.  Asserts the input
    conditions: every e_ref finite, every block that is not exactly zero has m >= 2**-100, and (where ll and y are present) every row's float64 gap
    between its two largest ll >= 2 * FORWARD_F x the row's block denominator of ll."""
    if key in _FWD_REF_CACHE:
        return _FWD_REF_CACHE[key]
    old, threads = torch.get_default_dtype(), torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    res = {}
    try:
        for dt in (torch.float64, torch.float32):
            torch.set_default_dtype(dt)
            with torch.no_grad():
                o = build(dt)
            assert all(v.dtype == dt for v in o.values() if v.is_floating_point()), "the oracle left %s" % dt
            res[dt] = o
    finally:
        torch.set_default_dtype(old)
        torch.set_num_threads(threads)
    fl = lambda o: {k: v.numpy().astype(np.float64) for k, v in o.items() if v.is_floating_point()}
    o64, o32 = fl(res[torch.float64]), fl(res[torch.float32])
    ref = dict(o64=o64, o32=o32, in32={k: v for k, v in res[torch.float32].items()}, m={}, e_ref={}, den={}, floor={},
               y={k: v.numpy() for k, v in res[torch.float64].items() if not v.is_floating_point()})
    for k, a in o64.items():
        m, e = step_blocks(a), step_blocks(o32[k] - a)
        assert np.isfinite(e).all() and np.isfinite(m).all(), "input condition: %s has a block whose e_ref is not finite" % k
        assert (m[m > 0] >= STEP_MIN_REF).all(), "input condition: %s has a non-zero block with a maximum below 2**-100" % k
        ref["m"][k], ref["e_ref"][k], ref["den"][k] = m, e, np.maximum(e, STEP_EPS * m)
        ref["floor"][k] = float(((e < STEP_EPS * m) & (m > 0)).sum()) / max(1, int((m > 0).sum()))
    for e in ("r", "n"):
        if "y_" + e in ref["y"]:
            ll = o64["ll_" + e]
            top = np.sort(ll, axis=1)
            gap, den = top[:, -1] - top[:, -2], ref["den"]["ll_" + e][0, np.arange(ll.shape[0]) // 16, 0]
            ok = gap >= 2 * FORWARD_F * den
            assert ok.all(), "input condition: row %d of ll_%s has a float64 gap of %.3e < 2 F x %.3e (change the case's seed)" % (
                int(np.argmin(ok)), e, gap[int(np.argmin(ok))], den[int(np.argmin(ok))])
            assert np.array_equal(ref["y"]["y_" + e], ll.argmax(1))
    _FWD_REF_CACHE[key] = ref
    return ref


def _canonical(fw, tr):
    """the oracle's forward dict and trace by the names of MODEL_OUTPUTS / ENGINE_BUFFERS, per-step tensors time-major"""
    o = {k: fw[k] for k in MODEL_OUTPUTS + Y_OUTPUTS if k in fw}
    for k in ("out", "r_out", "n_out"):
        if k in o:
            o[k] = _tm(o[k])
    o.update(tr)
    if "logits" in tr:
        T, B, _ = tr["logits"].shape
        o["logits_pad"] = torch.zeros(T, B, LOGIT_LD - E_VOCAB, dtype=tr["logits"].dtype)
    return {k: v.contiguous() for k, v in o.items()}


def gmvae_forward_references(case, sd, b, eps):
    """references of the whole forward of a GMVAE case (weights sd: CPU float32 state dict, batch dict b, eps = (eps_r, eps_n) CPU float32)"""
    d, r, n = (torch.as_tensor(b[k]).long() for k in ("d", "r", "n"))

    def build(dt):
        fw, tr = orc.forward({k: v.to(dt) for k, v in sd.items()}, d, r, n, torch.as_tensor(b["c"]).to(dt), eps[0].to(dt), eps[1].to(dt), trace=True)
        return _canonical(fw, tr)
    return forward_references(("forward", case["id"]), build)


def decoder_references(case, sd, b, zc, steps):
    """references of global_decoder(zc, steps) teacher forced with the batch's tokens; zc: CPU float32, an input of both sides"""
    d = torch.as_tensor(b["d"]).long()

    def build(dt):
        tr = {}
        out = orc.global_decoder({k: v.to(dt) for k, v in sd.items()}, zc.to(dt), steps, teacher=d[:, :steps], trace=tr)
        return _canonical({"out": out}, tr)
    return forward_references(("decoder", case["id"], steps), build)


def attr_references(case, sd, b, z_r, z_n):
    """references of sub_decoders(rhythm, z_r, note, z_n); z_r, z_n: CPU float32, inputs of both sides"""
    def build(dt):
        w, tr = {k: v.to(dt) for k, v in sd.items()}, {}
        fw = {"r_out": orc.sub_decoder(w, "r", orc.convert_to_one_hot(torch.as_tensor(b["r"]).long(), orc.R), z_r.to(dt), tr),
              "n_out": orc.sub_decoder(w, "n", orc.convert_to_one_hot(torch.as_tensor(b["n"]).long(), orc.N), z_n.to(dt), tr)}
        return _canonical(fw, tr)
    return forward_references(("attr", case["id"]), build)


# ---- the check ---------------------------------------------------------------------------------------------------------------------------
def check_forward_outputs(got, ref, F=None, names=None):
    """{name: array or tensor} of the forward under test (per-step tensors [steps][B][C]) against forward_references(), block by block:
      ratio   e <= F * max(e_ref, 2**-24 m) in every (step, 16 x 32) block with m > 0;
      zeros   a block with m == 0 is exactly zero (logits_pad: columns 342..351 of the logits buffer);
      y       y_r / y_n equal the float64 argmax in every row.
    names: the quantities this path must deliver (default: every reference quantity); a missing or an extra one is an error.
    Returns dict(worst=(ratio, name, step, (bi, bj)), per={name: (ratio, step, (bi, bj))}, floor={name: share}, blocks, zero_blocks)."""
    F = FORWARD_F if F is None else F
    assert F <= FORWARD_F_CAP
    names = tuple(ref["o64"]) + tuple(ref["y"]) if names is None else tuple(names)
    assert set(got) == set(names), sorted(set(got) ^ set(names))
    bad, per, blocks, zero_blocks = [], {}, 0, 0
    for k in names:
        a = got[k].detach().cpu().numpy() if torch.is_tensor(got[k]) else np.asarray(got[k])
        if k in Y_OUTPUTS:
            want = ref["y"][k]
            assert a.shape == want.shape, (k, a.shape, want.shape)
            rows = np.nonzero(a != want)[0]
            if len(rows):
                bad.append("%s: row %d is %d, the float64 argmax is %d (%d such rows)" % (k, rows[0], a[rows[0]], want[rows[0]], len(rows)))
            continue
        o64, m, den = ref["o64"][k], ref["m"][k], ref["den"][k]
        a = a.astype(np.float64)
        assert a.shape == o64.shape, (k, a.shape, o64.shape)
        e, mag = step_blocks(a - o64), step_blocks(a)
        zero = m == 0
        blocks += m.size
        zero_blocks += int(zero.sum())
        nz = zero & ~(mag == 0)
        if nz.any():
            t, bi, bj = (int(x) for x in np.argwhere(nz)[0])
            bad.append("%s: step %d block (%d, %d) is exactly zero in float64 and holds %.3e (%d such blocks)" % (k, t, bi, bj, mag[t, bi, bj], int(nz.sum())))
        ratio = np.where(zero, 0.0, e / np.where(zero, 1.0, den))
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        t, bi, bj = (int(x) for x in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        per[k] = (float(ratio[t, bi, bj]), t, (bi, bj))
        if not ratio[t, bi, bj] <= F:
            bad.append("%s: step %d block (%d, %d) err %.3e = %.1f x max(e_ref %.3e, 2**-24 x %.3e) (%d of %d blocks over F = %g)" % (
                k, t, bi, bj, e[t, bi, bj], ratio[t, bi, bj], ref["e_ref"][k][t, bi, bj], m[t, bi, bj], int((~(ratio <= F)).sum()), ratio.size, F))
    assert not bad, "\n".join(bad)
    wk = max(per, key=lambda k: per[k][0])
    return dict(worst=(per[wk][0], wk) + per[wk][1:], per=per, floor={k: ref["floor"][k] for k in per}, blocks=blocks, zero_blocks=zero_blocks)


def old_metric_accepts(got, ref):
    """What the suite asserted about the forward so far (_fw_check in test_gpu_parity.py, check_eval_side in helpers.py), with o32 in the place of the
    reference's own float32 outputs: elementwise |got - o32| <= 1e-4 + 1e-4 |o32| and equal y.  The suite applied it to the model's tuple only; here
    it is applied to every quantity in `got`, the engine's buffers included - more than the suite ever asked.  True = it accepts."""
    for k, v in got.items():
        a = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        if k in Y_OUTPUTS:
            if not np.array_equal(a, ref["y"][k]):
                return False
        elif not np.allclose(a, ref["o32"][k], rtol=1e-4, atol=1e-4):
            return False
    return True


def forward_line(path, case, arith, kernels, st):
    """one line of profiles/forward_fp64_errors.txt"""
    ratio, name, t, (bi, bj) = st["worst"]
    fl = max(st["floor"], key=lambda k: st["floor"][k])
    return "%-8s %-2s %-7s %-60s worst %-16s step %2d block (%2d, %2d) ratio %6.3f  floor share %.3f (highest: %s %.3f)" % (
        path, case, arith, kernels, name, t, bi, bj, ratio, st["floor"][name], fl, st["floor"][fl])


# ---- running a path --------------------------------------------------------------------------------------------------------------------------
def _buf(eng, name, shape):
    key = (eng.buf_ns + name, tuple(int(s) for s in shape), torch.float32)
    assert key in eng._bufs, "the engine has no buffer %s" % (key,)
    return eng._bufs[key]


def engine_buffers(eng, names, B, T=None, Tr=None):
    """the engine's named buffers behind `names`, by the names and shapes Engine gives them"""
    H, Z = eng.H, eng.Z
    o = {}
    for k in names:
        if k in ("pre_r", "pre_n"):
            o[k] = _buf(eng, k, (B, 2 * Z))
        elif k.startswith("enc_h_"):
            o[k] = _buf(eng, k, (T, B, H))[T - 1]
        elif k in ("h0g", "rbg"):
            o[k] = _buf(eng, "g_h0" if k == "h0g" else "g_rb", (B, H if k == "h0g" else 3 * H))
        elif k in ("hx0", "hx1", "gx2"):
            o[k] = _buf(eng, "g_" + k, (T, B, 3 * H if k == "gx2" else H))
        elif k in ("logits", "logits_pad"):
            lg = _buf(eng, "g_logits", (T * B, LOGIT_LD)).view(T, B, LOGIT_LD)
            o[k] = lg[:, :, :E_VOCAB] if k == "logits" else lg[:, :, E_VOCAB:]
        elif k.startswith("sd_h0_"):
            o[k] = _buf(eng, k, (B, H))
        elif k.startswith("sd_h_"):
            o[k] = _buf(eng, k, (Tr, B, H))
        elif k.startswith("sd_logits_"):
            o[k] = _buf(eng, k, (Tr, B, 3 if k.endswith("_r") else 16))
    return {k: v.detach().cpu().clone() for k, v in o.items()}


def tuple_outputs(res):
    """the model's nested tuple by the names of MODEL_OUTPUTS + Y_OUTPUTS, per-step tensors time-major"""
    (out, r_out, n_out, _, _), (dis_r, dis_n), (z_r, z_n), (ll_r, ll_n), (qy_r, qy_n), (y_r, y_n) = res
    o = dict(out=_tm(out), r_out=_tm(r_out), n_out=_tm(n_out), mu_r=dis_r.mean, sigma_r=dis_r.stddev, mu_n=dis_n.mean, sigma_n=dis_n.stddev,
             z_r=z_r, z_n=z_n, ll_r=ll_r, ll_n=ll_n, qy_r=qy_r, qy_n=qy_n, y_r=y_r, y_n=y_n)
    return {k: v.detach().cpu().clone() for k, v in o.items()}


def engine_tuple(eng, S):
    """the model's tuple from what Engine.forward left: the log-softmax launches of _forward_only on the logits"""
    ops, Z = eng.ops, eng.Z
    (B, T), Tr = S["d"].shape, S["r"].shape[1]
    dev = S["d"].device
    dec, lat, pre = S["dec"], S["lat"], S["pre"]
    out, r_out, n_out = torch.empty(B, T, E_VOCAB, device=dev), torch.empty(B, Tr, 3, device=dev), torch.empty(B, Tr, 16, device=dev)
    ops.vocab_logsoftmax(dec["logits"], B, T, E_VOCAB, logp_bt=out)
    ops.time_logsoftmax(dec["sd"]["r"]["logits"], logp_bt=r_out)
    ops.time_logsoftmax(dec["sd"]["n"]["logits"], logp_bt=n_out)
    o = dict(out=_tm(out), r_out=_tm(r_out), n_out=_tm(n_out), y_r=lat["r"]["y"].long(), y_n=lat["n"]["y"].long())
    for e in ("r", "n"):
        o["mu_" + e], o["sigma_" + e], o["z_" + e], o["ll_" + e], o["qy_" + e] = pre[e][:, :Z], lat[e]["sigma"], lat[e]["z"], lat[e]["ll"], lat[e]["qy"]
    return {k: v.detach().cpu().clone() for k, v in o.items()}


def run_forward_path(path, case, ops=None, device="cpu", arith=None, calls=1):
    """one call of a path of FORWARD_PATHS on a case -> (got, references, engine): seeded weights, synth_batch inputs, eps drawn after
    manual_seed(99) (helpers_step.gmvae_trainer); the latent inputs of the decoder and attribute paths are the float32 oracle's.
    calls > 1 (engine paths): that many calls in a row on the same engine, got = [the outputs of each]"""
    tr, eng, b, batch, eps = gmvae_trainer(case, ops=ops, device=device, arith=arith)
    m = tr.model
    sd = cpu_state(m)
    d, r, n, c, _, _, lab = batch
    (B, T), Tr = d.shape, r.shape[1]
    ref = gmvae_forward_references(case, sd, b, tuple(e.cpu() for e in eps))
    names = PATH_NAMES[path]
    if path in ("engine", "saved"):
        every = []
        for _ in range(calls):
            S = eng.forward(d, r, n, c, eps[0], eps[1], lab, save=path == "saved", head=True)
            assert (eng.saved is S) == (path == "saved")
            got = engine_tuple(eng, S)
            for k, t in (("hx1", S["dec"]["hx1"]), ("pre_n", S["pre"]["n"]), ("sd_h_r", S["dec"]["sd"]["r"]["h_all"])):      # the buffers read below are those of this call
                assert _buf(eng, {"hx1": "g_hx1"}.get(k, k), t.shape).data_ptr() == t.data_ptr()
            got.update(engine_buffers(eng, ENGINE_BUFFERS, B, T, Tr))
            every.append(got)
        return (got if calls == 1 else every), ref, eng
    with torch.no_grad():
        assert m.training
        if path == "dropin":
            got = tuple_outputs(m(d, r, n, c, eps=eps))
            got.update(engine_buffers(eng, ENGINE_BUFFERS, B, T, Tr))
        elif path == "encode":
            dis_r, dis_n = m.encode(d)
            got = {k: v.detach().cpu().clone() for k, v in (("mu_r", dis_r.mean), ("sigma_r", dis_r.stddev), ("mu_n", dis_n.mean), ("sigma_n", dis_n.stddev))}
            got.update(engine_buffers(eng, ENC_BUFFERS, B, T, Tr))
        elif path == "decoder":
            m(d, r, n, c, eps=eps)                                  # sets self.sample, as the reference's train-mode forward does
            zc = torch.cat([ref["in32"]["z_r"], ref["in32"]["z_n"], torch.as_tensor(b["c"]).float()], dim=1)
            out = m.global_decoder(zc.to(device), T - 1)
            ref = decoder_references(case, sd, b, zc, T - 1)
            got = {"out": _tm(out).detach().cpu().clone()}
            got.update(engine_buffers(eng, DEC_BUFFERS, B, T - 1))
        elif path == "attr":
            z_r, z_n = ref["in32"]["z_r"], ref["in32"]["z_n"]
            r_out, n_out, _, _ = m.sub_decoders(r, z_r.to(device), n, z_n.to(device))
            ref = attr_references(case, sd, b, z_r, z_n)
            got = {"r_out": _tm(r_out).detach().cpu().clone(), "n_out": _tm(n_out).detach().cpu().clone()}
            got.update(engine_buffers(eng, SD_BUFFERS, B, Tr=Tr))
        else:
            raise KeyError(path)
    assert set(got) == set(names)
    return got, ref, eng


# ---- which kernels a forward-only call ran ---------------------------------------------------------------------------------------------------
GATED_KERNELS = ("gru_fwd_pp_kernel", "gru_fwd_x6_kernel", "gru_fwd_x6pp_kernel")        # need saved gates (csrc/gru_plan.h)


def check_forward_only_kernels(launches, case):
    """launches: [(tags, step counts, persistent asked, [candidate kernel names in order], [fits per candidate: True / False / None], chosen index)]
    of one forward-only call - from the library's plans of the real launches (StepRecorder on the GPU) or from fn_gru_fwd_plan at 256 compute
    units on made-up addresses (planned_launches, no device: fits unknown, the first candidate counts as chosen).  Asserted:
      - no chosen kernel needs saved gates, whatever arithmetic was requested;
      - case g: every pipeline launch of two or more steps takes a weight-stationary gru_fwd_persist_kernel<...>;
      - the per-step kernel only where every weight-stationary candidate in front of it does not fit, or persist_dec is off (case e: then always).
    Returns a label for the profile lines."""
    assert launches, "no scan launch was recorded"
    seen = set()
    for tags, steps, persistent, cands, fits, chosen in launches:
        kern = cands[chosen]
        seen.add(kern)
        assert not kern.startswith(GATED_KERNELS), (tags, steps, kern)
        pipeline = any(t in ("dec_l1", "dec_l2") for t in tags)
        decoder = any(t.startswith(("dec_", "sd_")) for t in tags)
        if decoder and not case["persist"] and persistent is False:
            assert kernel_family(kern) == "step", (tags, kern)
            continue
        if case["id"] == "g" and pipeline and min(steps) >= 2:
            assert kern.startswith("gru_fwd_persist_kernel<"), (tags, steps, kern)
        if kernel_family(kern) == "step":
            assert all(f is False for f in fits[:chosen]), (tags, steps, cands, fits)
    if not case["persist"]:
        assert any(p is False for _, _, p, _, _, _ in launches)
    return "+".join(sorted(re.sub(r"^gru_|_kernel", "", k) for k in seen))


def recorded_launches(rec):
    """the launches of a helpers_step.StepRecorder in the form check_forward_only_kernels reads"""
    assert len(rec.fwd) == len([l for l in rec.launches if l[0] == "fwd"]) and not rec.bwd
    out = []
    for (way, tags, steps, persistent), p in zip(rec.launches, rec.fwd):
        assert p["status"] == 0 and p["chosen"] is not None and p["candidates"][p["chosen"]]["fits"] is not False, p
        out.append((tags, steps, persistent, [c["kernel"] for c in p["candidates"]], [c["fits"] for c in p["candidates"]], p["chosen"]))
    return out


def make_launch_log(base):
    """a stand-in class (FakeOps) that keeps the descriptors of every gru_seq_fwd launch: .log = [(descriptors, persistent asked)]"""
    class LaunchLog(base):
        def __init__(self):
            super().__init__()
            self.log = []

        def gru_seq_fwd(self, scans, **kw):
            self.log.append(([dict(s) for s in scans], kw.get("persistent", True)))
            super().gru_seq_fwd(scans, **kw)
    return LaunchLog


def planned_launches(log, x6=False):
    """fn_gru_fwd_plan at 256 compute units for every logged launch, with made-up addresses (helpers.lib_scan_candidates: the plan reads NULL-ness
    and alignment only) and gates as the launch had them -> the form check_forward_only_kernels reads; a refused launch has no candidate"""
    out = []
    for scans, persistent in log:
        desc = [dict(s, gates=s.get("gates") is not None) for s in scans]
        cands = lib_scan_candidates(desc, x6=x6, persistent=persistent, cus=256)[0]
        out.append((tuple(s.get("tag", "enc") for s in scans), tuple(s["T"] for s in scans), persistent, cands, [None] * len(cands), 0))
    return out
