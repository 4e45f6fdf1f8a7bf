"""Eval-mode global decoder: greedy autoregressive decode (gmm_model.py:119-149 with model.eval(), i.e.
``out = self._sampling(out)`` feedback, :147-148) and the fader-shift drivers of test_class.py:233-254,
:282-303 / arousal_transfer.ipynb cells 11+15, batched over many samples x fader values.

Per step: layer-1 cell (token row gather + recurrent MFMA GEMM + gates), layer-2 cell, 512->342 output
GEMM, log_softmax + first-index argmax written straight into the token matrix the next step reads.
"""
import numpy as np
import torch

from .constrain import Constraints, constraint_buffers, constraint_stats, load_constraints
from .engine import E_VOCAB, LOGIT_LD


def _is_int(v):
    """an int that is no bool"""
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_finite(v):
    """a finite real number that is no bool"""
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)) and bool(np.isfinite(v))


def _check_steps(steps, bools=True):
    """bools: True counts as the int it is (beam_decode refuses it)"""
    if not (isinstance(steps, (int, np.integer)) if bools else _is_int(steps)) or steps < 1:
        raise ValueError("steps: a positive int, got %r" % (steps,))


def _force_mask(force, steps):
    """force as greedy_decode takes it - a bool per step, or an int P = the first P steps - as a list of `steps` bools; ValueError otherwise"""
    _check_steps(steps)
    if _is_int(force):
        if not 0 <= int(force) <= steps:
            raise ValueError("force = P forces the first P steps: 0 <= P <= %d, got %d" % (steps, int(force)))
        return [i < int(force) for i in range(steps)]
    mask = np.asarray(force.detach().cpu() if torch.is_tensor(force) else force)
    if mask.ndim != 1 or mask.shape[0] != steps:
        raise ValueError("force: one entry per step (%d), got shape %s" % (steps, tuple(mask.shape)))
    return [bool(m) for m in mask]


def _forced_args(z, steps, forced, force):
    """validated (forced int32 (Bi, steps) on z's device, mask = tuple of `steps` bools with the ignored last entry False); ValueError
    before anything is launched"""
    if forced is None or force is None:
        raise ValueError("forced and force go together: the tokens and the per-step mask that selects them")
    _check_steps(steps)
    if not torch.is_tensor(forced):
        forced = torch.as_tensor(np.asarray(forced))
    if forced.is_floating_point() or forced.is_complex() or forced.dtype == torch.bool:
        raise ValueError("forced: integer tokens, got %s" % forced.dtype)
    if forced.dim() != 2 or forced.shape[0] != z.shape[0] or forced.shape[1] < steps:
        raise ValueError("forced: (%d, >= %d) tokens, got %s" % (z.shape[0], steps, tuple(forced.shape)))
    mask = _force_mask(force, steps)
    mask[steps - 1] = False                          # nothing is fed after the last step
    forced = forced[:, :steps]
    if forced.numel():
        lo, hi = int(forced.min()), int(forced.max())                  # a forced token indexes the embedding table
        if lo < 0 or hi >= E_VOCAB:
            raise ValueError("forced: tokens in [0, %d), got %d .. %d" % (E_VOCAB, lo, hi))
    return forced.to(device=z.device, dtype=torch.int32).contiguous(), tuple(mask)


def fed_tokens(tokens, forced, force):
    """the stream that was fed back: forced[b][i] where force[i], else the decoder's own token; force as greedy_decode takes it (a bool
    per step or an int P)"""
    m = torch.tensor(_force_mask(force, tokens.shape[1]), dtype=torch.bool, device=tokens.device)
    return torch.where(m.view(1, -1), forced[:, :tokens.shape[1]].to(device=tokens.device, dtype=tokens.dtype), tokens)


BEAM_MAX_WIDTH = 16        # FN_BEAM_MAX_W of include/fadernets.h
MAX_MASKED_GRAPHS = 4      # cached decode graphs whose key carries a mask (the unmasked ones are bounded by the shapes in use)


def _constraints_arg(constraints, Bi, eos=None, beam=False):
    """None or the validated Constraints of a decode of Bi sequences; ValueError before anything is launched"""
    if constraints is None:
        return None
    if not isinstance(constraints, Constraints):
        raise ValueError("constraints: None or a Constraints, got %r" % (constraints,))
    constraints.bias_rows(Bi)                  # a per-row bias has one row per sequence
    if beam and constraints.eos is not None and constraints.eos != eos:
        raise ValueError("constraints.eos (%d) is the beam's eos (%r) or None" % (constraints.eos, eos))
    return constraints


def _reset_constraints(con):
    """a decode starts: zeroes the counters and the sounding-pitch words of the buffers of constraint_buffers -> the words, or None where there are none"""
    if con is None:
        return None
    con["stuck"].zero_(), con["fixed"].zero_()
    if con["held"] is not None:
        con["held"].zero_()
    return con["held"]


def _prompt_arg(z, steps, prompt):
    """validated (the prompt (Bi, P <= steps) widened to (Bi, steps) CPU tokens, zeros behind it; P)"""
    prompt = prompt if torch.is_tensor(prompt) else torch.as_tensor(np.asarray(prompt))
    if prompt.dim() != 2 or prompt.shape[0] != z.shape[0] or prompt.shape[1] > steps:
        raise ValueError("prompt: (%d, <= %d) tokens, got %s" % (z.shape[0], steps, tuple(prompt.shape)))
    P = prompt.shape[1]
    full = torch.zeros(z.shape[0], steps, dtype=prompt.dtype)
    full[:, :P] = prompt.cpu()
    return full, P


def _init_state(eng, rows, prefix):
    """the two GEMMs in front of every decode, from the latent rows (z, or z repeated per beam) into the engine's buffers prefix + "h0g" / "rbg":
    (the global decoder's initial state, layer 1's per-row input bias)"""
    P, H = eng.p, eng.H
    h0g = eng.buf(prefix + "h0g", (rows.shape[0], H))
    eng.ops.gemm(rows, P["linear_init_global.weight"], h0g, bias=P["linear_init_global.bias"])
    rbg = eng.buf(prefix + "rbg", (rows.shape[0], 3 * H))
    eng.ops.gemm(rows, P["grucell_g.weight_ih"][:, E_VOCAB:], rbg)
    return h0g, rbg


def _arith_key(eng):
    """the cells' / GEMMs' arithmetic switches that select launches: a part of every graph key (a new switch goes here, once)"""
    ops = eng.ops
    return (bool(getattr(ops, "dw_x6", False) and getattr(ops, "cell_x6", False)), getattr(ops, "cell_x6_rows", None),
            bool(getattr(ops, "x6_per_tile", False)), bool(getattr(ops, "nt_x6", True)))


def _token_buffers(z, steps, want_logp, forced=None, params=None, con=None):
    """every tensor a captured greedy / sampling decode reads or writes, at its final size: copies of the inputs (zs, fs, ps, cb) and the results"""
    return dict(zs=z.clone(), fs=None if forced is None else forced.clone(), ps=None if params is None else params.to(z.device),
                cb=None if con is None else constraint_buffers(con, z.shape[0], z.device),
                tokens=torch.zeros(z.shape[0], steps, dtype=torch.int32, device=z.device),
                logp=torch.empty(z.shape[0], steps, E_VOCAB, device=z.device) if want_logp else None)


def _graph_replay(eng, cache, key, build, body, bounded, inputs, con=None, repeat=1):
    """One hipGraph per key in `cache`, captured at the key's first use and replayed on the given inputs -> (clones of the result buffers, cb).
    build() -> dict of the static buffers at their final sizes, "cb" among them (the buffers of constraint_buffers, or None); body(bufs, warm): the
    launches on them - first the warm-up (warm=True: a short run that allocates every scratch buffer at its FINAL size, nothing is allocated inside the
    capture), then the capture.  Every entry keeps its static buffers, so of the keys with bounded(key) at most MAX_MASKED_GRAPHS stay: the oldest
    goes.  inputs: buffer name -> this call's value, copied in before the replay together with the constraints' setting (con, repeat)."""
    ent = cache.get(key)
    if ent is None:
        bufs = build()
        body(bufs, True)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        getattr(eng.ops, "begin_capture", lambda: None)()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            body(bufs, False)
        ent = cache[key] = (g, bufs)
        old = [k for k in cache if bounded(k)]
        if len(old) > MAX_MASKED_GRAPHS:
            del cache[old[0]]
    g, bufs = ent
    for name, v in inputs.items():
        if bufs[name] is not None:
            bufs[name].copy_(v)
    if bufs["cb"] is not None:
        load_constraints(bufs["cb"], con, inputs["zs"].shape[0], repeat)
    g.replay()
    return {k: (None if v is None else v.clone()) for k, v in bufs.items() if k not in inputs and k != "cb"}, bufs["cb"]


@torch.no_grad()
def greedy_decode(model, z, steps, want_logp=True, use_graph=None, forced=None, force=None, constraints=None):
    """z (Bi, 2Z+24) -> (log-probs (Bi, steps, 342) or None, tokens (Bi, steps) int32).

    forced (Bi, >= steps) integer tokens + force (a bool per step, or an int P = the first P steps): after step i the decoder is fed
    forced[:, i] instead of its own argmax wherever force[i] (gmm_model.py:139-144 with force[i] = `p < self.eps`; a prompt is a prefix).
    The results keep their meaning: the model's OWN log-probs and first-index argmax of every step (fed_tokens() gives the fed stream).

    Bi <= Engine.single_launch_rows: ONE launch for the whole decode (fn_decode_greedy; above 32 rows a pipeline of 32- / 64-row blocks through
    its role workgroups).  Larger batches: steps x {layer-1 cell, W_ih2 projection,
    layer-2 cell, output GEMM, log_softmax+argmax} (from Engine.cell_decode_rows sequences on: steps x {layer-1 cell, layer-2 cell incl.
    its projection - fn_gru_cell_f32 -, output GEMM, argmax}; with want_logp=False: {layer-1 cell, layer-2 cell, output layer with the
    argmax in its epilogue - fn_out_argmax_f32}) captured once per (Bi, steps) into a hipGraph and replayed.  The captured
    kernels read the parameters and the engine's weight images IN PLACE (stable addresses, refreshed by Engine.refresh_weights
    after every optimiser step / load_state_dict), so a graph stays valid when the weights change.

    constraints: None or a Constraints - every step's logits go through fn_constrain_apply before the head and the token that is FED (the forced
    one at a forced step) through fn_constrain_advance after it, so the log-probs and tokens are those of the constrained distribution (banned
    entries exactly -inf); want_stats appends dict(stuck, fixed).  Limitation: a constrained decode takes the per-token launches only - never the
    one-launch kernels fn_decode_greedy / fn_decode_forced and never the fused output layer fn_out_argmax_f32, which feed back their own argmax."""
    eng = model.engine()
    z = z.float().contiguous()
    mask = None
    if forced is not None or force is not None:
        forced, mask = _forced_args(z, steps, forced, force)
    con = _constraints_arg(constraints, z.shape[0])
    if con is not None:
        _check_steps(steps)
    if con is None and _single_launch_ok(eng, z):
        res = _decode_single_launch(eng, z, steps, want_logp, forced, mask)
        if res is not None:
            return res
    if use_graph is None:
        # a graph per mask: by default only for the masks that come back (none, a prompt prefix); an arbitrary mask - every scheduled-sampling
        # step draws a new one - goes launch by launch unless the caller asks for the graph
        use_graph = z.is_cuda and (mask is None or not any(b and not a for a, b in zip(mask, mask[1:])))
    if not use_graph:
        cb = None if con is None else constraint_buffers(con, z.shape[0], z.device)
        logp, tokens = _decode_body(eng, z, steps, want_logp, None, None, forced=forced, mask=mask, con=cb)
        return (logp, tokens, constraint_stats(cb)) if con is not None and con.want_stats else (logp, tokens)
    # the captured launches depend on the path taken, on the cells' / GEMMs' arithmetic switches, on the form of the constraints and - the per-token
    # paths pick every step's token pointer on the host - on the mask; the unmasked graphs are bounded by the shapes in use
    key = (z.shape[0], steps, bool(want_logp), decode_path(eng, z.shape[0], want_logp, None, con), *_arith_key(eng),
           None if con is None else con.key(), mask)
    out, cb = _graph_replay(eng, eng.__dict__.setdefault("_decode_graphs", {}), key, lambda: _token_buffers(z, steps, want_logp, forced, con=con),
                            lambda b, warm: _decode_body(eng, b["zs"], min(steps, 2) if warm else steps, want_logp, b["logp"], b["tokens"],
                                                         alloc_steps=steps, forced=b["fs"], mask=mask, con=b["cb"]),
                            lambda k: k[-1] is not None, dict(zs=z, fs=forced), con)
    logp, tokens = out["logp"], out["tokens"]
    return (logp, tokens, constraint_stats(cb)) if con is not None and con.want_stats else (logp, tokens)


def continue_from(model, z, prompt, steps, want_logp=True, constraints=None):
    """Prompted continuation: prompt (Bi, P) tokens, 0 <= P <= steps -> (log-probs (Bi, steps, 342) or None, tokens (Bi, steps) int32) where
    tokens[:, :P] is the prompt and the rest is what the model wrote after it (the stream that was fed back); the log-probs are
    the model's own at every step, i.e. logp[:, i] scores tokens[:, i] given the start token and tokens[:, :i].  constraints: as greedy_decode."""
    forced, P = _prompt_arg(z, steps, prompt)
    if P == 0:
        return greedy_decode(model, z, steps, want_logp, constraints=constraints)
    res = greedy_decode(model, z, steps, want_logp, forced=forced, force=P, constraints=constraints)
    res[1][:, :P] = forced[:, :P].to(device=res[1].device, dtype=res[1].dtype)
    return res


def _sample_args(z, steps, temperature, top_k, top_p, seed, offset, prompt):
    """validated (the 32 bytes of FnSampleParams as a CPU uint8 tensor, prompt int32 (Bi, steps) on z's device or None, its prefix mask or None, P);
    ValueError before anything is launched"""
    _check_steps(steps)
    for name, v in (("temperature", temperature), ("top_p", top_p)):
        if not _is_finite(v):
            raise ValueError("%s: a finite number, got %r" % (name, v))
    if not temperature > 0:
        raise ValueError("temperature > 0, got %r" % (temperature,))
    if not 0 < top_p <= 1:
        raise ValueError("0 < top_p <= 1, got %r" % (top_p,))
    for name, v, hi in (("top_k", top_k, 1 << 31), ("seed", seed, 1 << 64), ("offset", offset, 1 << 64)):
        if not _is_int(v) or not 0 <= int(v) < hi:
            raise ValueError("%s: an int in [0, 2^%d), got %r" % (name, hi.bit_length() - 1, v))
    P, forced, mask = 0, None, None
    if prompt is not None:
        full, P = _prompt_arg(z, steps, prompt)
        if P:
            forced, mask = _forced_args(z, steps, full, P)
    with np.errstate(over="ignore"):
        inv_t = np.float32(1.0) / np.float32(temperature)          # the kernel clamps what fp32 cannot hold
    raw = np.zeros(1, dtype=[("seed", "<u8"), ("offset", "<u8"), ("inv_t", "<f4"), ("top_p", "<f4"), ("top_k", "<i4"), ("reserved", "<i4")])
    raw["seed"], raw["offset"], raw["inv_t"], raw["top_p"], raw["top_k"] = int(seed), int(offset), inv_t, np.float32(top_p), int(top_k)
    return torch.from_numpy(raw.view(np.uint8).copy()), forced, mask, P


@torch.no_grad()
def sample_decode(model, z, steps, temperature=1.0, top_k=0, top_p=1.0, seed=0, offset=0, want_logp=True, prompt=None, use_graph=None,
                  constraints=None):
    """Seeded temperature / top-k / top-p sampling: z (Bi, 2Z+24) -> (log-probs (Bi, steps, 342) or None, tokens (Bi, steps) int32).

    tokens is the stream that was fed back: the draws, with tokens[:, :P] = prompt (Bi, P <= steps) when one is given; the log-probs are the
    model's own, untempered, of every step: logp.gather(-1, tokens) scores the sample.  Step i of row b draws with the uniform
    Philox4x32-10(key = seed, counter = (b, i, offset)) from the distribution include/fadernets.h defines at fn_vocab_sample: softmax(logits /
    temperature) restricted to the top_k most likely tokens (0: all), then to the shortest prefix of them that holds top_p of their mass.
    The same (seed, offset) gives the same uniforms on every path and batch size, and the same tokens on the same path (the paths' logits differ
    in their low bits); top_k = 1 is greedy_decode.

    The reference has no counterpart (its _sampling is the argmax, gmm_model.py:73-80).  Every batch size takes the per-token launches -
    scan steps below Engine.cell_decode_rows rows, cells from there on - with the output GEMM and fn_vocab_sample as the head; the
    one-launch decode kernel is not involved.  On the GPU the launches are captured once per (Bi, steps, want_logp, P, arithmetic) into
    Engine._sample_graphs (at most MAX_MASKED_GRAPHS of them with a prompt: the oldest goes); z, the prompt and the 32 parameter bytes are copied
    into the graph's buffers, so any seed or setting replays it.

    constraints: None or a Constraints, as greedy_decode takes it: the draw is from the constrained distribution (a banned token has weight 0) and the
    log-probs are that distribution's.  fn_constrain_advance replaces a drawn token that is banned after all - the draw counts fp32 prefix sums, see
    include/fadernets.h - by the row's argmax, so a banned token is never fed; want_stats appends dict(stuck, fixed).  The graph's key gains
    Constraints.key(); the 32 parameter bytes and the bias are copied into its buffers."""
    params, forced, mask, P = _sample_args(z, steps, temperature, top_k, top_p, seed, offset, prompt)
    con = _constraints_arg(constraints, z.shape[0])
    eng = model.engine()
    z = z.float().contiguous()
    cb = None
    if use_graph is None:
        use_graph = z.is_cuda
    if not use_graph:
        cb = None if con is None else constraint_buffers(con, z.shape[0], z.device)
        logp, tokens = _decode_body(eng, z, steps, want_logp, None, None, forced=forced, mask=mask, sample=params.to(z.device), con=cb)
    else:
        key = (z.shape[0], steps, bool(want_logp), P, decode_path(eng, z.shape[0], want_logp, params, con), None if con is None else con.key(), *_arith_key(eng))
        out, cb = _graph_replay(eng, eng.__dict__.setdefault("_sample_graphs", {}), key, lambda: _token_buffers(z, steps, want_logp, forced, params, con),
                                lambda b, warm: _decode_body(eng, b["zs"], min(steps, 2) if warm else steps, want_logp, b["logp"], b["tokens"],
                                                             alloc_steps=steps, forced=b["fs"], mask=mask, sample=b["ps"], con=b["cb"]),
                                lambda k: k[3], dict(zs=z, ps=params, fs=forced), con)          # bounded: the graphs with a prompt, as greedy_decode's masked ones
        logp, tokens = out["logp"], out["tokens"]
    if P:
        tokens[:, :P] = forced[:, :P]
    return (logp, tokens, constraint_stats(cb)) if con is not None and con.want_stats else (logp, tokens)


def _beam_args(steps, width, eos, length_penalty):
    """validated (W, eos as the kernels take it: -1 = none, length_penalty as a float); ValueError before anything is launched"""
    _check_steps(steps, bools=False)
    if not _is_int(width) or not 1 <= int(width) <= BEAM_MAX_WIDTH:
        raise ValueError("width: an int in [1, %d], got %r" % (BEAM_MAX_WIDTH, width))
    if eos is not None and (not _is_int(eos) or not 0 <= int(eos) < E_VOCAB):
        raise ValueError("eos: None or a token in [0, %d), got %r" % (E_VOCAB, eos))
    if not _is_finite(length_penalty):
        raise ValueError("length_penalty: a finite number, got %r" % (length_penalty,))
    return int(width), -1 if eos is None else int(eos), float(length_penalty)


def _beam_buffers(z, W, steps, keep_logp, con=None):
    """every tensor the beam loop writes, at its final size (nothing is allocated inside a capture); cb: the constraints' buffers, or None"""
    Bi, dev = z.shape[0], z.device
    i32 = dict(dtype=torch.int32, device=dev)
    return dict(zs=z.clone(), cb=None if con is None else constraint_buffers(con, Bi, dev, repeat=W, gather=True), score=torch.zeros(steps, Bi, W, device=dev), parent=torch.zeros(steps, Bi, W, **i32), token=torch.zeros(steps, Bi, W, **i32),
                rows=torch.empty(steps, Bi * W, E_VOCAB, device=dev) if keep_logp else None,
                tokens=torch.zeros(Bi, W, steps, **i32), beam=torch.zeros(Bi, W, steps, **i32), cum=torch.zeros(Bi, W, steps, device=dev),
                lens=torch.zeros(Bi, W, **i32), final=torch.zeros(Bi, W, device=dev))


def _beam_body(eng, bufs, W, steps, eos, run_steps=None, con=None):
    """the launches of beam_decode on the buffers of _beam_buffers: per step {layer-1 cell, layer-2 cell with its projection, output GEMM, fn_beam_step,
    fn_beam_gather}, then one fn_beam_backtrack.  The cells write the `cur` states, the gather writes the states the next step reads (rows reordered by
    parent beam); layer 1's gx_rowbias is the same for all beams of a sequence and needs no reorder.  run_steps < steps: a warm-up of the first steps.
    con: None, or the buffers of constraint_buffers - then fn_constrain_apply runs on the Bi*W rows in front of fn_beam_step, the sounding-pitch words
    travel through the gather as a third job (4 columns, the words carried as floats: the copy moves all 32 bits) and fn_constrain_advance moves
    them by the step's tokens."""
    ops, P, H = eng.ops, eng.p, eng.H
    z = bufs["zs"]
    R = z.shape[0] * W
    zr = eng.buf("beam_z", (R, z.shape[1]))
    zr.view(z.shape[0], W, z.shape[1]).copy_(z.unsqueeze(1).expand(z.shape[0], W, z.shape[1]))
    h0g, rbg = _init_state(eng, zr, "beam_")
    cur0, cur1, nxt0, nxt1 = (eng.buf("beam_" + n, (R, H)) for n in ("cur0", "cur1", "nxt0", "nxt1"))
    logits = eng.buf("beam_logits", (R, LOGIT_LD))
    score, parent, token, rows = bufs["score"], bufs["parent"], bufs["token"], bufs["rows"]
    n = steps if run_steps is None else min(steps, run_steps)
    held = _reset_constraints(con)
    for i in range(n):
        ops.gru_cell(h0g if i == 0 else nxt0, P["grucell_g.weight_hh"], P["grucell_g.bias_hh"], cur0, b_ih=P["grucell_g.bias_ih"], gx_table=eng.tab["g"],
                     start_token=E_VOCAB - 1, gx_rowbias=rbg, idx=token[i - 1].view(-1) if i > 0 else None)
        ops.gru_cell(cur0 if i == 0 else nxt1, P["grucell_g_2.weight_hh"], P["grucell_g_2.bias_hh"], cur1, x=cur0, w_ih=P["grucell_g_2.weight_ih"],
                     b_ih=P["grucell_g_2.bias_ih"])
        ops.gemm(cur1, P["linear_out_g.weight"], logits[:, :E_VOCAB], bias=P["linear_out_g.bias"])
        if con is not None:
            ops.constrain_apply(logits, E_VOCAB, i, con["params"], bias=con["bias"], held=held, stuck=con["stuck"])
        ops.beam_step(logits, W, E_VOCAB, i, eos, score[i - 1] if i > 0 else None, token[i - 1] if i > 0 else None, score[i], parent[i], token[i],
                      logp_out=None if rows is None else rows[i])
        if i + 1 < steps:          # nothing reads the states of the last step
            if held is None:
                ops.beam_gather([(cur0, nxt0), (cur1, nxt1)], parent[i].view(-1), W)
            else:
                ops.beam_gather([(cur0, nxt0), (cur1, nxt1), (held.view(torch.float32), con["held_g"].view(torch.float32))], parent[i].view(-1), W)
                ops.constrain_advance(token[i].view(-1), E_VOCAB, con["params"], held_in=con["held_g"], held_out=held)
    if n == steps:
        ops.beam_backtrack(parent, token, score, eos, bufs["tokens"], bufs["lens"], bufs["final"], beam_out=bufs["beam"], cum_out=bufs["cum"])


@torch.no_grad()
def beam_decode(model, z, steps, width=4, eos=None, length_penalty=0.0, want_logp=False, use_graph=None, trace=False, constraints=None):
    """Beam search to width W: z (Bi, 2Z+24) -> (tokens (Bi, W, steps) int32, scores (Bi, W) fp32, lengths (Bi, W) int32), the W most likely token
    sequences the search finds under each latent, best first; scores are the summed log-probs (fp32, include/fadernets.h at fn_beam_step has the
    exact arithmetic and the tie order: higher score, then lower beam, then lower token).

    eos: None, or a token that ends a hypothesis - it is then extended by eos at no cost, so the positions after its end hold eos, its score stays
    and lengths = 1 + the first position holding eos (steps where there is none).  length_penalty != 0 re-sorts the W hypotheses of a latent by
    score / length ** length_penalty (stable; the scores returned stay the sums).  want_logp: a fourth result (Bi, W, steps, 342), the model's own
    log-probs along each returned hypothesis (the row that scored its token at every step; after a hypothesis' end: the model fed eos).  trace=True
    appends a dict of the raw slabs score / parent / token (steps, Bi, W), rows (steps, Bi*W, 342) = every step's log-prob rows, beam / cum
    (Bi, W, steps) and order (Bi, W), all but order in the kernels' order (before the length_penalty sort).  width = 1 is a greedy decode.

    The reference has no counterpart (its loop feeds one argmax stream, gmm_model.py:73-80,119-149).  Every batch size takes Bi*W rows (z repeated
    W-fold) through per-token launches: the two fn_gru_cell_f32 cells, the output GEMM, fn_beam_step and fn_beam_gather per step, one
    fn_beam_backtrack at the end.  On the GPU the loop is captured once per (Bi, W, steps, eos, log-probs kept, arithmetic) into Engine._beam_graphs
    (at most MAX_MASKED_GRAPHS stay, the oldest goes) and replayed on a copy of z.  Not covered: a prompt with beams, and the one-launch decode
    kernel (it feeds back its own argmax).

    constraints: None or a Constraints (its eos None or the beam's): every beam row's logits go through fn_constrain_apply, each beam carries its
    own sounding pitches (reordered by parent with the decoder states), and scores, log-probs and the trace rows are those of the constrained
    distribution.  A sequence with fewer than W allowed continuations yields hypotheses of score -inf; they are reported as they are.  A per-row bias
    has one row per latent, shared by its W beams.  want_stats appends dict(stuck, fixed) over the Bi*W beam rows (fixed stays 0) as the last result."""
    W, eos_k, lpen = _beam_args(steps, width, eos, length_penalty)
    con = _constraints_arg(constraints, z.shape[0], eos, beam=True)
    eng = model.engine()
    z = z.float().contiguous()
    keep = bool(want_logp or trace)
    if use_graph is None:
        use_graph = z.is_cuda
    if not use_graph:
        bufs = _beam_buffers(z, W, steps, keep, con)
        cb = bufs["cb"]
        _beam_body(eng, bufs, W, steps, eos_k, con=cb)
    else:
        key = (z.shape[0], W, steps, eos_k, keep, None if con is None else con.key(), *_arith_key(eng))
        bufs, cb = _graph_replay(eng, eng.__dict__.setdefault("_beam_graphs", {}), key, lambda: _beam_buffers(z, W, steps, keep, con),
                                 lambda b, warm: _beam_body(eng, b, W, steps, eos_k, run_steps=2 if warm else None, con=b["cb"]),
                                 lambda k: True, dict(zs=z), con, repeat=W)          # bounded: all of them, every entry owns static slabs (and log-prob rows)
    tokens, scores, lens, beam = bufs["tokens"], bufs["final"], bufs["lens"], bufs["beam"]
    Bi = z.shape[0]
    order = torch.arange(W, device=z.device).view(1, W).expand(Bi, W)
    if lpen != 0.0:
        order = torch.sort(-(scores / lens.to(scores.dtype) ** lpen), dim=1, stable=True)[1]
    ar = torch.arange(Bi, device=z.device).view(Bi, 1)
    res = [tokens[ar, order], scores[ar, order], lens[ar, order]]
    if want_logp:
        rows = bufs["rows"].view(steps, Bi, W, E_VOCAB)
        b = beam[ar, order].long()                                                      # (Bi, W, steps)
        res.append(rows[torch.arange(steps, device=z.device).view(1, 1, steps), ar.view(Bi, 1, 1), b])
    if trace:
        res.append(dict(score=bufs["score"], parent=bufs["parent"], token=bufs["token"], rows=bufs["rows"], beam=beam, cum=bufs["cum"], order=order))
    if con is not None and con.want_stats:
        res.append(constraint_stats(cb))
    return tuple(res)


def _single_launch_ok(eng, z):
    """small batches decode as ONE launch (fn_decode_greedy: weight slices resident in LDS, activations handed over through L2)"""
    lo, hi = getattr(eng, "single_launch_skip", (0, -1))
    return (hasattr(eng.ops, "decode_greedy") and z.is_cuda and z.shape[0] <= eng.single_launch_rows and not (lo <= z.shape[0] <= hi)
            and eng.H <= 512 and eng.single_launch_decode)


def decode_path(eng, Bi, want_logp, sample, con):
    """the per-token path _decode_body takes for Bi sequences: "scan_steps" (below Engine.cell_decode_rows: scan-step kernels + projection GEMM),
    "cells" (fn_gru_cell_f32 cells, output GEMM, a head launch) or "cells_fused" (the cells with the argmax in the output layer's epilogue,
    fn_out_argmax_f32: tokens only, no sampling, no constraints).  sample / con: None or not, as _decode_body takes them."""
    if Bi < eng.cell_decode_rows:
        return "scan_steps"
    fused = not want_logp and sample is None and con is None and getattr(eng, "fused_argmax", True) and hasattr(eng.ops, "out_argmax")
    return "cells_fused" if fused else "cells"


def _single_launch_args(eng, h0g, rbg, steps, tokens, logp, forced=None, mask=None):
    """the arguments of HipOps.decode_greedy / decode_plan on the initial state h0g and layer 1's row bias rbg (_init_state)"""
    P = eng.p
    # forced feedback (fn_decode_forced): the mask travels as device bytes, the kernel reads it step by step
    fkw = {} if mask is None else dict(forced=forced, force=torch.tensor(mask, dtype=torch.uint8).to(tokens.device))
    return (h0g.shape[0], steps, eng.H, E_VOCAB, E_VOCAB - 1, eng.whh_f["g"], P["grucell_g.bias_hh"], P["grucell_g.bias_ih"], eng.tab["g"], rbg, h0g,
            eng.packs["ih2"], P["grucell_g_2.bias_ih"], eng.whh_f["g2"], P["grucell_g_2.bias_hh"], eng.packs["out"], P["linear_out_g.bias"], tokens,
            logp), fkw


def single_launch_plan(eng, Bi, steps, want_logp=True, forced=None, mask=None):
    """what the one-launch decode of Bi sequences launches on this engine (HipOps.decode_plan on the arguments _decode_single_launch hands to
    decode_greedy; the state buffers are the ones _init_state fills, unfilled), or None where it is not eligible on this device.  Nothing is enqueued."""
    tokens = torch.zeros(Bi, steps, dtype=torch.int32, device=eng.dev)
    logp = torch.empty(Bi, steps, E_VOCAB, device=eng.dev) if want_logp else None
    args, fkw = _single_launch_args(eng, eng.buf("dec_h0g", (Bi, eng.H)), eng.buf("dec_rbg", (Bi, 3 * eng.H)), steps, tokens, logp, forced, mask)
    return eng.ops.decode_plan(*args, **fkw)


def _decode_single_launch(eng, z, steps, want_logp, forced=None, mask=None):
    """None when the library reports the configuration as not eligible (e.g. fewer CUs than role workgroups) or the launch
    timed out waiting for a hand-over: the caller then takes the per-token path."""
    ops = eng.ops
    Bi = z.shape[0]
    h0g, rbg = _init_state(eng, z, "dec_")
    tokens = torch.zeros(Bi, steps, dtype=torch.int32, device=z.device)
    logp = torch.empty(Bi, steps, E_VOCAB, device=z.device) if want_logp else None
    args, fkw = _single_launch_args(eng, h0g, rbg, steps, tokens, logp, forced, mask)
    ok = ops.decode_greedy(*args, **fkw)
    if not ok:
        return None
    if ops.gru_sync_error(clear=True):           # bounded spin gave up (another kernel held the CUs): results are garbage
        import warnings
        warnings.warn("single-launch greedy decode timed out waiting for a hand-over; repeating on the per-token kernels")
        return None
    return logp, tokens


def _decode_body(eng, z, steps, want_logp, logp, tokens, alloc_steps=None, forced=None, mask=None, sample=None, con=None):
    """sample: None, or the 32 device bytes of FnSampleParams - then `tokens` receives the DRAWN tokens (fn_vocab_sample in place of the argmax
    launch, never the fused output layer), which are what the next step is fed; forced / mask keep their meaning (a prompt).
    con: None, or the buffers of constraint_buffers - then every step is {output GEMM, fn_constrain_apply, the head, fn_constrain_advance on the token
    that is fed: the forced column at a forced step (state only), else tokens[:, i] with the fix-up}, never the fused output layer.  The advance is
    left out where it can do nothing: no sounding-pitch state and either a forced token or the argmax head, whose token is never a banned one."""
    ops, P, H = eng.ops, eng.p, eng.H
    Bi = z.shape[0]
    dev = z.device
    if tokens is None:
        tokens = torch.zeros(Bi, steps, dtype=torch.int32, device=dev)
    if logp is None and want_logp:
        logp = torch.empty(Bi, steps, E_VOCAB, device=dev)
    hx0 = [eng.buf("dec_hx0_a", (1, Bi, H)), eng.buf("dec_hx0_b", (1, Bi, H))]
    hx1 = [eng.buf("dec_hx1_a", (1, Bi, H)), eng.buf("dec_hx1_b", (1, Bi, H))]
    h0g, rbg = _init_state(eng, z, "dec_")
    gx2 = eng.buf("dec_gx2", (1, Bi, 3 * H))
    logits = eng.buf("dec_logits", (Bi, LOGIT_LD))
    # every cell also leaves its new state in the MFMA operand layout, which the next cell call takes as h0_frag: no packing launches
    nf = ops.frag_floats(Bi, H)
    hf0 = [eng.buf("dec_hf0_a", (nf,)), eng.buf("dec_hf0_b", (nf,))]
    hf1 = [eng.buf("dec_hf1_a", (nf,)), eng.buf("dec_hf1_b", (nf,))]

    held = _reset_constraints(con)

    def head(i):
        if con is not None:
            ops.constrain_apply(logits, E_VOCAB, i, con["params"], bias=con["bias"], held=held, stuck=con["stuck"])
        if sample is None:
            ops.vocab_argmax(logits, E_VOCAB, logp[:, i, :] if want_logp else None, tokens[:, i])
        elif con is None:
            ops.vocab_sample(logits, E_VOCAB, sample, i, logp[:, i, :] if want_logp else None, tokens[:, i])
        else:
            ops.vocab_sample(logits, E_VOCAB, sample, i, logp[:, i, :] if want_logp else None, tokens[:, i], own_out=con["own"])
        if con is None:
            return
        if mask is not None and mask[i]:
            if held is not None:
                ops.constrain_advance(forced[:, i], E_VOCAB, con["params"], held_in=held, held_out=held)
        elif sample is not None:
            ops.constrain_advance(tokens[:, i], E_VOCAB, con["params"], logits=logits, fallback=con["own"], held_in=held, held_out=held, fixed=con["fixed"])
        elif held is not None:
            ops.constrain_advance(tokens[:, i], E_VOCAB, con["params"], held_in=held, held_out=held)

    path = decode_path(eng, Bi, want_logp, sample, con)
    if path != "scan_steps":
        # thousands of rows: every cell is ONE MFMA launch with the gates in its epilogue (fn_gru_cell_f32: LDS-free loop above 512 rows); layer 2 takes its input
        # projection in the same K loop - 3 launches + argmax per token instead of 4 + argmax, and no [B][3H] round trip
        # tokens only (the evaluators' sweeps): the output layer takes the argmax into its epilogue (fn_out_argmax_f32: packed (logit, column)
        # words by 64-bit atomic max, no logits, no argmax launch) and the next layer-1 cell reads its token from the packed word -
        # 3 launches per token; the int32 tokens are unpacked once at the end
        fused = path == "cells_fused"
        best = eng.buf("dec_best", (max(steps, alloc_steps or 0), Bi), dtype=torch.int64)[:steps] if fused else None
        if fused:
            best.zero_()
        for i in range(steps):
            cur, prv = i & 1, (i & 1) ^ 1
            if mask is not None and i > 0 and mask[i - 1]:      # forced step: the previous token is a given one
                tok_src = dict(idx=forced[:, i - 1])
            else:
                tok_src = dict(idx_best=best[i - 1], best_v=E_VOCAB) if fused and i > 0 else dict(idx=tokens[:, i - 1] if i > 0 else None)
            ops.gru_cell(h0g if i == 0 else hx0[prv][0], P["grucell_g.weight_hh"], P["grucell_g.bias_hh"], hx0[cur][0], b_ih=P["grucell_g.bias_ih"],
                         gx_table=eng.tab["g"], start_token=E_VOCAB - 1, gx_rowbias=rbg, **tok_src)
            ops.gru_cell(hx0[cur][0] if i == 0 else hx1[prv][0], P["grucell_g_2.weight_hh"], P["grucell_g_2.bias_hh"], hx1[cur][0],
                         x=hx0[cur][0], w_ih=P["grucell_g_2.weight_ih"], b_ih=P["grucell_g_2.bias_ih"])
            if fused:
                ops.out_argmax(hx1[cur][0], P["linear_out_g.weight"], P["linear_out_g.bias"], best[i])
            else:
                ops.gemm(hx1[cur][0], P["linear_out_g.weight"], logits[:, :E_VOCAB], bias=P["linear_out_g.bias"])
                head(i)
        if fused:
            ops.best_tokens(best, E_VOCAB, tokens)
        return logp, tokens
    for i in range(steps):
        cur, prv = i & 1, (i & 1) ^ 1
        ops.gru_seq_fwd([dict(B=Bi, T=1, H=H, w_hh_frag=eng.whh_f["g"], b_hh=P["grucell_g.bias_hh"], b_ih=P["grucell_g.bias_ih"],
                              h0=h0g if i == 0 else hx0[prv][0], h0_frag=None if i == 0 else hf0[prv], h_last_frag=hf0[cur],
                              gx_table=eng.tab["g"], idx=forced if mask is not None and i > 0 and mask[i - 1] else tokens, idx_shift=i - 1,
                              start_token=E_VOCAB - 1, gx_rowbias=rbg, h_all=hx0[cur])], persistent=False)
        ops.gemm(hx0[cur][0], P["grucell_g_2.weight_ih"], gx2[0], bias=P["grucell_g_2.bias_ih"])
        ops.gru_seq_fwd([dict(B=Bi, T=1, H=H, w_hh_frag=eng.whh_f["g2"], b_hh=P["grucell_g_2.bias_hh"],
                              h0=hx0[cur][0] if i == 0 else hx1[prv][0], h0_frag=hf0[cur] if i == 0 else hf1[prv], h_last_frag=hf1[cur],
                              gx_dense=gx2, h_all=hx1[cur])], persistent=False)
        ops.gemm(hx1[cur][0], P["linear_out_g.weight"], logits[:, :E_VOCAB], bias=P["linear_out_g.bias"])
        head(i)
    return logp, tokens


def clean_output(out):
    """test_class.py:44-50: argmax over the vocabulary -> trim zeros at both ends -> cut at the first EOS (token 1).
    Accepts log-probs (1, steps, 342) or an int token row."""
    if torch.is_tensor(out) and out.is_floating_point():
        recon = torch.argmax(out, dim=-1).cpu().numpy().squeeze()
    else:
        recon = np.asarray(out.cpu() if torch.is_tensor(out) else out).squeeze()
    recon = np.trim_zeros(np.atleast_1d(recon))
    if 1 in recon:
        last = np.argwhere(recon == 1)[0][0]
        recon[recon == 1] = 0
        recon = recon[:last]
    return recon


def _check_beam(steps, prompt, sample, beam):
    if beam is not None:
        if sample is not None or prompt is not None:
            raise ValueError("beam goes with neither sample nor prompt")
        unknown = set(beam) - {"width", "eos", "length_penalty"}
        if unknown:
            raise ValueError("beam: keys among width, eos, length_penalty; got %s" % sorted(unknown, key=str))
        _beam_args(steps, beam.get("width", 4), beam.get("eos"), beam.get("length_penalty", 0.0))


def _decode_rows(model, z, steps, prompt=None, sample=None, beam=None, constraints=None):
    """the decode fader_sweep's keywords select, over the rows of z -> tokens (rows, steps) int32"""
    rows = z.shape[0]
    pr = None if prompt is None else (prompt if torch.is_tensor(prompt) else torch.as_tensor(np.asarray(prompt))).reshape(1, -1)
    if beam is not None:
        return beam_decode(model, z, steps, constraints=constraints, **beam)[0][:, 0].contiguous()
    if sample is not None:
        unknown = set(sample) - {"temperature", "top_k", "top_p", "seed", "offset"}
        if unknown:
            raise ValueError("sample: keys among temperature, top_k, top_p, seed, offset; got %s" % sorted(unknown, key=str))
        return sample_decode(model, z, steps, want_logp=False, prompt=None if pr is None else pr.expand(rows, pr.shape[1]), constraints=constraints,
                             **sample)[1]
    if prompt is None:
        return greedy_decode(model, z, steps, want_logp=False, constraints=constraints)[1]
    return continue_from(model, z, pr.expand(rows, pr.shape[1]), steps, want_logp=False, constraints=constraints)[1]


def fader_latents(model, dis_r, dis_n, amounts, eps=None, which="r", mode="set"):
    """The latent arithmetic of fader_sweep for an (n, V) matrix of amounts - one per (sample, value) pair, on the posteriors' device:
      mode="set":   z_which[i, v, 0] = amounts[i, v];   mode="shift": z_which[i, v] += amounts[i, v] * (mu_lookup[1] - mu_lookup[0])
    eps as fader_sweep takes it; None = drawn here (r first, then n).
    -> (zr, zn (n, V, Z) fresh tensors, z0 (n,) or (n, V): the value of z_which[:, 0] before the change; which="both": z_r's)"""
    n, Z = dis_r.mean.shape
    V = amounts.shape[1]
    dev = dis_r.mean.device
    if eps is None:
        eps = (torch.randn(n, Z), torch.randn(n, Z))      # repar() of test_class.py:53-56 draws r first, then n
    er, en = (e.to(dev).float() for e in eps)
    per_value = er.dim() == 3
    if not per_value:
        er, en = er.unsqueeze(1).expand(n, V, Z), en.unsqueeze(1).expand(n, V, Z)
    zr = dis_r.mean.unsqueeze(1) + dis_r.stddev.unsqueeze(1) * er          # (n, V, Z), fresh tensors
    zn = dis_n.mean.unsqueeze(1) + dis_n.stddev.unsqueeze(1) * en
    z0 = (zn if which == "n" else zr)[:, :, 0].clone()
    if not per_value:
        z0 = z0[:, 0]
    if mode == "set":
        (zr if which == "r" else zn)[:, :, 0] = amounts
    else:
        for tgt, lk, on in ((zr, model.mu_r_lookup, which in ("r", "both")), (zn, model.mu_n_lookup, which in ("n", "both"))):
            if on:
                tgt += amounts.unsqueeze(2) * (lk.weight.data[1] - lk.weight.data[0]).view(1, 1, Z)
    return zr, zn, z0


@torch.no_grad()
def fader_sweep(model, x, chroma, values, steps=100, which="r", eps=None, mode="set", prompt=None, sample=None, beam=None, constraints=None):
    """Batched RhythmEvaluator.shift / NoteEvaluator.shift (test_class.py:233-254, :282-303) and the notebook's
    lambda*shift-vector transfer (cells 11 + 15): every (sample, fader value) pair is one row of ONE decode batch.

    x (n, T) token ids or (n, T, 342) one-hot; chroma (n, 24); values: V fader values.
      mode="set":   z_which[:, 0] = value                                   (test_class.py:249, :298)
      mode="shift": z_which += value * (mu_lookup[1] - mu_lookup[0]);  which="both" moves z_r and z_n together, as the notebook does
    eps: (eps_r, eps_n), each (n, Z) - one draw per sample, shared by its V values - or (n, V, Z) - one draw per (sample, value),
    which is what V separate reference calls consume; None = drawn here (r first, then n).
    prompt: (P,) or (1, P) tokens every (sample, value) row starts with (continue_from), or None.
    sample: None = the greedy decode; a dict of sample_decode's keywords (temperature, top_k, top_p, seed, offset) = drawn continuations.
    beam: None, or a dict of beam_decode's keywords (width, eos, length_penalty) = every row's best hypothesis; not with sample or prompt.
    constraints: None, or a Constraints for whichever decode runs (a per-row bias has n * V rows; its want_stats is not reported here).
    Returns (tokens (n, V, steps) int32, z0 (n,) or (n, V): the value of z_which[:, 0] before the change; which="both": z_r's)."""
    if which not in ("r", "n", "both") or mode not in ("set", "shift") or (which == "both" and mode == "set"):
        raise ValueError("which in {r, n, both}, mode in {set, shift}; 'both' only with mode='shift'")
    _check_beam(steps, prompt, sample, beam)
    was_training = model.training
    model.eval()
    try:
        dis_r, dis_n = model.encode(x)
        n, V = dis_r.mean.shape[0], len(values)
        dev = dis_r.mean.device
        vals = torch.as_tensor(values, dtype=torch.float32, device=dev)
        zr, zn, z0 = fader_latents(model, dis_r, dis_n, vals.view(1, V).expand(n, V), eps, which, mode)
        c = chroma.float().to(dev).unsqueeze(1).expand(n, V, chroma.shape[-1])
        z = torch.cat([zr, zn, c], dim=2).reshape(n * V, -1)
        return _decode_rows(model, z, steps, prompt, sample, beam, constraints).view(n, V, steps), z0
    finally:
        model.train(was_training)
