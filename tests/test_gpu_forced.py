"""Forced-token feedback in decode on a real MI355X: fn_decode_forced in its three regimes (one block, 32-row pipeline, 64-row pipeline) and
the per-token paths (scan steps, fp32 cells, bf16 x 6 cells), each with a prefix mask, a seeded Bernoulli(0.5) mask and every step forced,
with and without log-probs, every replayed position checked by helpers_forced.replay_forced_check against an fp64 replay of the stream that
was fed (tolerance min(1e-4, 16 e_ref), cap 2 % as helpers.replay_decode_check)."""
import numpy as np
import pytest
import torch

from helpers import ONE_LAUNCH_BLOCKS, make_model, replay_inputs, replay_z
from helpers_forced import (FORCED_CASES, FORCED_GRAPH_PATHS, FORCED_MASKS, fed_stream, forced_line, forced_mask, forced_tokens,
                            replay_forced_check)
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _arith_tag(eng):
    return "bf16x6" if eng.ops.dw_x6 else "f32"


@pytest.mark.parametrize("path,weights,Bi,steps", FORCED_CASES, ids=["%s-%s-%d" % (p, w, b) for p, w, b, _ in FORCED_CASES])
def test_forced_decode_paths_every_step_vs_fp64_replay(path, weights, Bi, steps):
    pkg = load_package()
    from music_fader_nets_amd import decode as dec
    H, Z, sd = replay_inputs(weights)
    m = make_model(H, Z, sd, device=DEV, arith="bf16x6" if path == "cells_x6" else None)
    m.eval()
    eng = m.engine()
    one_launch = path in ("one_launch", "pipeline32", "pipeline64")
    if one_launch:
        eng.single_launch_decode, eng.single_launch_skip = True, (0, -1)
        if Bi > eng.single_launch_rows:
            eng.single_launch_rows = 2048
        # what the library launches for this engine's own tensors (fn_decode_plan, forced and not) is what the case's name says
        for fkw in ({}, dict(forced=forced_tokens(Bi, steps, Bi).to(device=DEV, dtype=torch.int32), mask=(True,) * steps)):
            plan = dec.single_launch_plan(eng, Bi, steps, **fkw)
            assert plan is not None and dec._single_launch_ok(eng, torch.empty(Bi, 1, device=DEV)) and plan["forced"] == bool(fkw)
            assert (plan["block_rows"], plan["nblk"]) == ONE_LAUNCH_BLOCKS[path](Bi) and (plan["nblk"] == 1) == (path == "one_launch"), (path, Bi, plan)
    elif path == "scan_steps":
        eng.single_launch_decode, eng.cell_decode_rows = False, 1 << 30
        assert dec.decode_path(eng, Bi, True, None, None) == "scan_steps" and dec.decode_path(eng, Bi, False, None, None) == "scan_steps"
    else:
        eng.single_launch_decode = False
        assert dec.decode_path(eng, Bi, True, None, None) == "cells" and dec.decode_path(eng, Bi, False, None, None) == "cells_fused"
        x6 = eng.ops.dw_x6 and eng.ops.cell_x6 and Bi >= eng.ops.cell_x6_rows
        assert x6 == (path == "cells_x6")
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    z = replay_z(Bi, Z, Bi)
    zd = z.to(DEV)
    forced = forced_tokens(Bi, steps, Bi)
    graphs = eng.__dict__.setdefault("_decode_graphs", {})
    tag = "%s[%s]/%s" % (path, _arith_tag(eng), weights)

    def decode(zz, want_logp, **kw):
        n = len(graphs)
        if kw and path in FORCED_GRAPH_PATHS:
            kw["use_graph"] = True                            # by default only unmasked and prefix masks are captured
        res = pkg.greedy_decode(m, zz, steps, want_logp=want_logp, **kw)
        assert not eng.ops.gru_sync_error()                  # the sticky error word, after every call
        assert not one_launch or len(graphs) == n             # the one-launch paths did not fall back to the per-token kernels
        return res

    # no step forced, through the forced entry point / the forced per-token code: the plain decode, bit for bit
    lp0, tk0 = decode(zd, True)
    lp1, tk1 = decode(zd, True, forced=forced, force=np.zeros(steps, bool))
    assert torch.equal(tk0, tk1) and torch.equal(lp0, lp1)
    _, tk0n = decode(zd, False)
    _, tk1n = decode(zd, False, forced=forced, force=0)
    assert torch.equal(tk0n, tk1n)
    for kind in FORCED_MASKS:
        force = forced_mask(kind, steps, Bi)
        lp, tk = decode(zd, True, forced=forced.to(DEV), force=force)
        _, tk_only = decode(zd, False, forced=forced, force=force)
        st = replay_forced_check(sd, z, tk, forced, force, pkg.fed_tokens(tk, forced, force), lp)
        print("\n" + forced_line(tag, kind, H, st), end="")
        if not torch.equal(tk_only, tk):
            st = replay_forced_check(sd, z, tk_only, forced, force, pkg.fed_tokens(tk_only, forced, force))
            print("\n" + forced_line(tag + " tokens", kind, H, st), end="")
        if path in FORCED_GRAPH_PATHS:                        # the cached graph of this mask on a second latent / forced batch
            n = len(graphs)
            z2, forced2 = replay_z(Bi, Z, Bi + 1), forced_tokens(Bi, steps, Bi + 1)
            lp2, tk2 = decode(z2.to(DEV), True, forced=forced2, force=force)
            assert len(graphs) == n
            st = replay_forced_check(sd, z2, tk2, forced2, force, fed_stream(tk2, forced2, force), lp2)
            print("\n" + forced_line(tag + " graph batch 2", kind, H, st), end="")
    # a second mask (the one-launch kernel reads it from device memory; the per-token paths capture it into a graph of its own)
    force2 = forced_mask("bernoulli", steps, Bi + 1)
    assert not np.array_equal(force2, forced_mask("bernoulli", steps, Bi))
    n = len(graphs)
    lp, tk = decode(zd, True, forced=forced, force=force2)
    if not one_launch:                                        # a graph of its own, and the cache of masked graphs stays capped
        want = tuple(bool(x) for x in force2[:-1]) + (False,)
        assert any(k[-1] == want for k in graphs) and sum(k[-1] is not None for k in graphs) <= dec.MAX_MASKED_GRAPHS
    st = replay_forced_check(sd, z, tk, forced, force2, fed_stream(tk, forced, force2), lp)
    print("\n" + forced_line(tag + " mask 2", "bernoulli", H, st))


def test_continue_from_and_prompted_sweep_on_the_default_dispatch():
    """continue_from on the default dispatch (one launch): the prompt, then what the model wrote after it; the log-probs score that stream"""
    pkg = load_package()
    H, Z, sd = replay_inputs("h512")
    m = make_model(H, Z, sd, device=DEV)
    m.eval()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    Bi, steps, P = 40, 64, 16
    z = replay_z(Bi, Z, 4)
    prompt = forced_tokens(Bi, P, 4)
    lp, tk = pkg.continue_from(m, z.to(DEV), prompt, steps)
    assert not m.engine().ops.gru_sync_error()
    assert torch.equal(tk[:, :P].cpu().long(), prompt)
    own = lp.argmax(-1).cpu()
    assert torch.equal(own[:, P:], tk[:, P:].cpu().long())
    forced = torch.zeros(Bi, steps, dtype=torch.long)
    forced[:, :P] = prompt
    replay_forced_check(sd, z, own, forced, np.arange(steps) < P, tk, lp)
    g = torch.Generator().manual_seed(8)
    x = torch.randint(0, 342, (5, 20), generator=g).to(DEV)
    tok, _ = pkg.fader_sweep(m, x, torch.rand(5, 24, generator=g).to(DEV), [-1.0, 0.0, 1.0, 2.0], steps=32, prompt=prompt[0])
    assert tuple(tok.shape) == (5, 4, 32) and torch.equal(tok[:, :, :P].cpu().long(), prompt[0].view(1, 1, P).expand(5, 4, P))


def test_forced_entry_point_answers_as_the_greedy_one():
    """shape / alignment answers of fn_decode_forced are fn_decode_greedy's; the new arguments' own: NULL and a short forced_ld"""
    import ctypes as C
    load_package()
    from music_fader_nets_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    itok = torch.zeros(64, dtype=torch.int32, device=DEV)
    msk = torch.zeros(8, dtype=torch.uint8, device=DEV)
    d = _lib.FnDecode()
    for nm in ("w_hh1_frag", "b_hh1", "table1", "h0", "w_ih2_frag", "w_hh2_frag", "b_hh2", "w_out_frag", "b_out", "ws", "sync_ws"):
        setattr(d, nm, buf.data_ptr())
    d.tokens, d.tok_ld = itok.data_ptr(), 8
    d.B, d.steps, d.H, d.V, d.start_token = 4, 8, 48, 342, 341             # H % 32 != 0
    f = _lib.FnDecodeForce()
    f.forced, f.forced_ld, f.force = itok.data_ptr(), 8, msk.data_ptr()
    assert lib.fn_decode_greedy(C.byref(d), None) == _lib.FN_E_SHAPE and lib.fn_decode_forced(C.byref(d), C.byref(f), None) == _lib.FN_E_SHAPE
    d.H = 64
    d.ws = buf.data_ptr() + 4
    assert lib.fn_decode_greedy(C.byref(d), None) == _lib.FN_E_ALIGN and lib.fn_decode_forced(C.byref(d), C.byref(f), None) == _lib.FN_E_ALIGN
    d.ws = buf.data_ptr()
    f.forced_ld = 7
    assert lib.fn_decode_forced(C.byref(d), C.byref(f), None) == _lib.FN_E_SHAPE
    f.forced_ld, f.force = 8, None
    assert lib.fn_decode_forced(C.byref(d), C.byref(f), None) == _lib.FN_E_NULL
