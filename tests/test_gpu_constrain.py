"""Constrained decode on a real MI355X: fn_constrain_apply / fn_constrain_advance bit for bit against the restatement on every case the CPU tests run
through the two statements and the host twin, fn_beam_gather moving the sounding-pitch words with all their bits, and greedy / sample / beam decodes
with a full constraint set on the scan-step and the cell paths: the fed stream against the automaton, the -inf pattern of the log-probs, an fp64
replay through the fp64 restatement, graph replay against eager, a second replay with other parameter bytes, and constraints that ban nothing
against the unconstrained call."""
import numpy as np
import pytest
import torch

from helpers import make_model, replay_inputs, replay_rows, replay_z
from helpers_constrain import (CASE_SHAPES, assert_stream_valid, bias_bans, constrained_replay_check, constraint_params, favour_note_offs,
                               full_constraints, kernel_cases, params_bytes, prompt_tokens, reference_case, same_result)
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = 342
STEPS = 24


def _ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(DEV)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy())


@pytest.mark.parametrize("rows,v", CASE_SHAPES, ids=["%dx%d" % s for s in CASE_SHAPES])
def test_constrain_kernels_alone(rows, v):
    """every case: the apply in place on a [rows][V + 5] matrix whose last columns are sentinels, counters that start above zero, a per-row bias that is
    a strided view, tokens and fallbacks that are strided views; then the advance on the rows the apply left"""
    ops = _ops()
    for c in kernel_cases(rows, v):
        ref = reference_case(c)
        prm = torch.from_numpy(params_bytes(c["p"])).to(DEV)
        xd = torch.from_numpy(c["x"]).to(DEV)
        bias = None
        if c["bias"] is not None and c["bias"].ndim == 2:
            wide = torch.full((rows, v + 3), float("nan"), device=DEV)
            wide[:, :v] = torch.from_numpy(c["bias"]).to(DEV)
            bias = wide[:, :v]
        elif c["bias"] is not None:
            bias = torch.from_numpy(c["bias"]).to(DEV)
        held = None if c["held"] is None else _i32(c["held"]).to(DEV)
        stuck = torch.full((rows,), 5, dtype=torch.int32, device=DEV)
        ops.constrain_apply(xd, v, c["step"], prm, bias=bias, held=held, stuck=stuck)
        tokb = torch.full((rows, 2), -9, dtype=torch.int32, device=DEV)
        fbb = torch.full((rows, 3), -9, dtype=torch.int32, device=DEV)
        tokb[:, 0], fbb[:, 1] = torch.from_numpy(c["tok"]).to(DEV), torch.from_numpy(c["fb"]).to(DEV)
        fixed = torch.full((rows,), 2, dtype=torch.int32, device=DEV)
        held_out = held if c["alias"] or held is None else torch.full((rows, 4), -1, dtype=torch.int32, device=DEV)
        ops.constrain_advance(tokb[:, 0], v, prm, logits=xd if c["fixup"] else None, fallback=fbb[:, 1] if c["fixup"] else None, held_in=held,
                              held_out=held_out, fixed=fixed)
        torch.cuda.synchronize()
        got = dict(logits=xd.cpu().numpy(), stuck=stuck.cpu().numpy() - 5, tok=tokb[:, 0].cpu().numpy(),
                   held=None if held is None else held_out.cpu().numpy(), fixed=fixed.cpu().numpy() - 2)
        same_result(got, ref, "%dx%d %s" % (rows, v, c["tag"]))
        assert bool((tokb[:, 1] == -9).all()) and bool((fbb[:, 0] == -9).all()) and bool((fbb[:, 2] == -9).all())
        if held is not None and not c["alias"]:
            assert np.array_equal(held.cpu().numpy().view(np.uint32), c["held"])               # held_in is only read
        # without the optional outputs: the same rows
        x2 = torch.from_numpy(c["x"]).to(DEV)
        ops.constrain_apply(x2, v, c["step"], prm, bias=bias, held=None if c["held"] is None else _i32(c["held"]).to(DEV))
        assert torch.equal(x2.view(torch.int32), xd.view(torch.int32))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset_4_bytes"])
def test_beam_gather_moves_every_bit_of_the_held_words(offset):
    """the sounding-pitch words travel through fn_beam_gather as floats: a NaN payload, all ones and a denormal survive bit for bit, on the 16-byte
    copies (an aligned view) and on the scalar copies (a view that starts 4 bytes in)"""
    ops = _ops()
    rows, W = 12, 4
    words = np.array([0x7fa00000, 0xffffffff, 0x00000001, 0x80000000], dtype=np.uint32)
    src = np.stack([np.roll(words, r) ^ np.uint32(r << 8) for r in range(rows)])
    src[:, 0] = words[np.arange(rows) % 3]
    parent = torch.tensor([3, 0, 0, 2, 1, 1, 1, 1, 0, 3, 2, 9], dtype=torch.int32)
    sb = torch.zeros(rows, 8, dtype=torch.int32, device=DEV)
    db = torch.full((rows, 8), 77, dtype=torch.int32, device=DEV)
    sb[:, offset:offset + 4] = _i32(src).to(DEV)
    ops.beam_gather([(sb.view(torch.float32)[:, offset:offset + 4], db.view(torch.float32)[:, offset:offset + 4])], parent.to(DEV), W)
    torch.cuda.synchronize()
    idx = (np.arange(rows) // W) * W + np.clip(parent.numpy(), 0, W - 1)
    got = db.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:, offset:offset + 4], src[idx])
    assert (np.delete(got, np.arange(offset, offset + 4), axis=1) == 77).all()
    for w in words[:3]:
        assert (got[:, offset:offset + 4] == w).any()


def _model(pkg, cells_from=None):
    H, Z, sd = replay_inputs("h64")
    m = make_model(H, Z, sd, device=DEV)
    m.eval()
    eng = m.engine()
    eng.single_launch_decode = False                      # the unconstrained comparisons stay on the per-token launches
    eng.cell_decode_rows = cells_from if cells_from is not None else 1 << 30
    return m, eng, {k: v.detach().cpu() for k, v in m.state_dict().items()}, Z


def _other(pkg, con, Bi):
    """another setting of the same key: another min_length, another bias, another ceiling"""
    bias = favour_note_offs(4.0)
    if con.bias_mode == 2:
        bias = bias.unsqueeze(0).repeat(Bi, 1)
        bias[::2, 178:200] += 1.0
    return pkg.Constraints(bias=bias, ban=(0, 300), min_length=17, eos=1, off_needs_on=True, no_reonset=True, max_polyphony=2, want_stats=True)


@pytest.mark.parametrize("mode", ["greedy", "sample"])
@pytest.mark.parametrize("path,Bi", [("scan_steps", 3), ("cells", 64)])
def test_constrained_decode_end_to_end(mode, path, Bi):
    pkg = load_package()
    m, eng, sd, Z = _model(pkg, 64 if path == "cells" else None)
    from music_fader_nets_amd import decode as dec
    # a constrained decode never takes the fused output layer: with and without log-probs, greedy or sampled, it is the path of the case's name
    for want_logp in (True, False):
        assert dec.decode_path(eng, Bi, want_logp, None if mode == "greedy" else object(), object()) == path
    z = replay_z(Bi, Z, Bi)
    zd = z.to(DEV)
    rows = replay_rows(Bi)
    prompt = prompt_tokens(Bi)
    full = torch.zeros(Bi, STEPS, dtype=torch.int64)
    full[:, :3] = prompt
    graphs = eng.__dict__.setdefault("_decode_graphs" if mode == "greedy" else "_sample_graphs", {})

    def run(c, **kw):
        if mode == "greedy":
            res = pkg.greedy_decode(m, zd, STEPS, forced=full, force=3, constraints=c, **kw)
            return res + (pkg.fed_tokens(res[1], full, 3),)
        res = pkg.sample_decode(m, zd, STEPS, temperature=1.3, seed=5, prompt=prompt, constraints=c, **kw)
        return res + (res[1],)

    def check(tag, con, res):
        logp, tokens, stats, fed = res
        assert not eng.ops.gru_sync_error() and tokens.dtype == torch.int32 and tuple(logp.shape) == (Bi, STEPS, V)
        assert int(stats["stuck"].sum()) == 0 and (mode == "sample" or int(stats["fixed"].sum()) == 0)
        p = constraint_params(con)
        st = assert_stream_valid(fed.cpu(), p, True, bias_bans(con, Bi), logp.cpu())
        assert st["max_poly_seen"] == con.max_polyphony and st["note_ons"] > Bi
        rep = constrained_replay_check(sd, z, fed.cpu(), logp.cpu(), p, True, con.bias, rows=rows, own=tokens.cpu() if mode == "greedy" else None)
        print("\n%-7s %-10s %-12s Bi %3d  e_ref %.3e  max|dlogp| %.3e  banned %.1f %%  fixed %d" % (
            mode, path, tag, Bi, rep["e_ref"], rep["max_dlp"], 100 * rep["banned_share"], int(stats["fixed"].sum())), end="")

    def same(a, b):
        for x, y in zip(a[:2], b[:2]):
            assert torch.equal(x, y)
        for k in ("stuck", "fixed"):
            assert torch.equal(a[2][k], b[2][k])

    con = full_constraints(pkg, per_row=Bi if path == "cells" else 0)
    res = run(con)
    n = len(graphs)
    check("graph", con, res)
    same(res, run(con, use_graph=False))                                    # launch by launch: the same, bit for bit
    # other parameter bytes and another bias through the cached graph
    con2 = _other(pkg, con, Bi)
    res2 = run(con2)
    assert len(graphs) == n and not torch.equal(res2[1], res[1])
    check("replay 2", con2, res2)
    same(res2, run(con2, use_graph=False))
    same(res, run(con))
    # constraints that ban nothing: the unconstrained call of the same path, bit for bit
    lp0, tk0, _ = run(None)
    lp1, tk1, _ = run(pkg.Constraints())
    assert torch.equal(tk0, tk1) and torch.equal(lp0, lp1) and bool(torch.isfinite(lp0).all()) and not torch.equal(tk0, res[1])
    print()


@pytest.mark.parametrize("Bi,W", [(2, 4), (16, 4)])
def test_constrained_beams_end_to_end(Bi, W):
    pkg = load_package()
    m, eng, sd, Z = _model(pkg)
    z = replay_z(Bi, Z, Bi)
    zd = z.to(DEV)
    rows = np.arange(Bi)
    graphs = eng.__dict__.setdefault("_beam_graphs", {})

    def run(c, **kw):
        return pkg.beam_decode(m, zd, STEPS, width=W, eos=1, want_logp=True, constraints=c, **kw)

    def check(tag, con, res):
        tokens, scores, lens, logp, stats = (r if isinstance(r, dict) else r.cpu() for r in res)
        assert tuple(tokens.shape) == (Bi, W, STEPS) and tuple(logp.shape) == (Bi, W, STEPS, V) and bool(torch.isfinite(scores).all())
        assert int(stats["stuck"].sum()) == 0 and int(stats["fixed"].sum()) == 0 and bool((scores[:, :-1] >= scores[:, 1:]).all())
        p = constraint_params(con)
        seen = 0
        for j in range(W):
            st = assert_stream_valid(tokens[:, j], p, True, bias_bans(con, Bi), logp[:, j])
            seen = max(seen, st["max_poly_seen"])
            rep = constrained_replay_check(sd, z, tokens[:, j], logp[:, j], p, True, con.bias, rows=rows, scores=scores[:, j], lens=lens[:, j])
            print("\nbeam %-10s Bi %2d W %d hypothesis %d  e_ref %.3e  max|dlogp| %.3e  max|dscore| %.3e" % (
                tag, Bi, W, j, rep["e_ref"], rep["max_dlp"], rep["max_dscore"]), end="")
        assert seen == con.max_polyphony

    def same(a, b):
        for x, y in zip(a[:4], b[:4]):
            assert torch.equal(x, y)
        assert torch.equal(a[4]["stuck"], b[4]["stuck"])

    con = full_constraints(pkg, per_row=Bi if Bi == 16 else 0)
    res = run(con)
    n = len(graphs)
    check("graph", con, res)
    same(res, run(con, use_graph=False))
    con2 = _other(pkg, con, Bi)
    res2 = run(con2)
    assert len(graphs) == n and not torch.equal(res2[0], res[0])
    check("replay 2", con2, res2)
    same(res2, run(con2, use_graph=False))
    same(res, run(con))
    plain, free = run(None), run(pkg.Constraints())
    for x, y in zip(plain, free):
        assert torch.equal(x, y)
    assert not torch.equal(plain[0], res[0]) and not eng.ops.gru_sync_error()
    print()
