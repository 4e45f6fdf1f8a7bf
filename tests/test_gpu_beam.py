"""Beam-search decode on a real MI355X: fn_beam_step alone (log-probs bit-equal to fn_vocab_argmax, slabs bit-equal to the definition on the kernel's
own log-prob rows, strided outputs), fn_beam_gather against torch indexing, fn_beam_backtrack against a numpy walk, decode.beam_decode end to end
(every step against the definition, returned hypotheses against an fp64 replay, cached graph / no graph, width 1, eos), the other decodes untouched."""
import numpy as np
import pytest
import torch

from helpers import make_model, replay_decode_check, replay_inputs, replay_z
from helpers_beam import (BEAM_CASES, STEP_SHAPES, beam_check_backtrack, beam_check_step, beam_check_trace, beam_line, beam_replay_check, beam_rows,
                          reference_backtrack, step_inputs)
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = 342


def _ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(DEV)


@pytest.mark.parametrize("B,W,v", STEP_SHAPES, ids=["%dx%dx%d" % s for s in STEP_SHAPES])
def test_beam_step_kernel_alone(B, W, v):
    ops = _ops()
    from music_fader_nets_amd.engine import LOGIT_LD
    R = B * W
    for step in (0, 5):
        for eos in (-1, min(1, v - 1)):
            x, sp, tp = step_inputs(B, W, v, step, eos, seed=300 + 10 * B + W, ld=LOGIT_LD if v == V else v + 3)
            xd = x.to(DEV)
            good = ~torch.isnan(x[:, :v]).any(1)
            lp_ref = torch.full((R, 3, v), 7.0, device=DEV)
            ops.vocab_argmax(xd, v, lp_ref[:, 1, :], torch.zeros(R, dtype=torch.int32, device=DEV))
            # every slab is a strided slice of a larger sentinel-filled tensor
            spb, tpb = torch.full((B, 2, W + 1), 3.0, device=DEV), torch.full((B, 2, W + 1), -3, dtype=torch.int32, device=DEV)
            spb[:, 1, :W], tpb[:, 1, :W] = sp.to(DEV), tp.to(DEV)
            prev = (spb[:, 1, :W], tpb[:, 1, :W]) if step else (None, None)
            lp = torch.full((R, 3, v), 7.0, device=DEV)
            sc = torch.full((B, 3, W + 2), 9.0, device=DEV)
            pa, tk = (torch.full((B, 3, W + 2), -5, dtype=torch.int32, device=DEV) for _ in range(2))
            ops.beam_step(xd, W, v, step, eos, prev[0], prev[1], sc[:, 1, :W], pa[:, 1, :W], tk[:, 1, :W], logp_out=lp[:, 1, :])
            torch.cuda.synchronize()
            lpc, refc = lp.cpu(), lp_ref.cpu()
            assert torch.equal(lpc[good], refc[good]) and bool(torch.isnan(lpc[~good][:, 1]).all())          # bit for bit with the greedy head
            assert bool((lpc[:, 0] == 7.0).all()) and bool((lpc[:, 2] == 7.0).all())
            beam_check_step(lpc[:, 1].numpy(), W, step, eos, sp, tp, sc[:, 1, :W].cpu(), pa[:, 1, :W].cpu(), tk[:, 1, :W].cpu())
            for t, fill in ((sc, 9.0), (pa, -5), (tk, -5)):
                assert int((t == fill).sum()) == t.numel() - B * W
            assert bool((spb[:, 0] == 3.0).all()) and torch.equal(spb[:, 1, :W].cpu(), sp) and torch.equal(tpb[:, 1, :W].cpu(), tp)
            # log-probs not wanted: the same slabs
            sc2, pa2, tk2 = torch.zeros(B, W, device=DEV), torch.zeros(B, W, dtype=torch.int32, device=DEV), torch.zeros(B, W, dtype=torch.int32, device=DEV)
            ops.beam_step(xd, W, v, step, eos, prev[0], prev[1], sc2, pa2, tk2)
            assert torch.equal(sc2.view(torch.int32), sc[:, 1, :W].contiguous().view(torch.int32)) and torch.equal(pa2, pa[:, 1, :W]) and torch.equal(tk2, tk[:, 1, :W])


@pytest.mark.parametrize("rows,W,H", [(20, 4, 64), (48, 16, 512), (7, 1, 96), (2048, 8, 512)])
def test_beam_gather(rows, W, H):
    """two jobs in one launch: 16-byte aligned views of padded matrices (the vector copies) and views that start one float in (the scalar copies);
    parents include values to clamp"""
    ops = _ops()
    g = torch.Generator().manual_seed(rows)
    parent = torch.randint(0, W, (rows,), generator=g, dtype=torch.int32)
    parent[::7] = W + 2
    parent[3::11] = -1
    a = torch.randn(rows, H + 4, generator=g).to(DEV)
    b = torch.randn(rows, H + 3, generator=g).to(DEV)
    da, db = torch.full((rows, H + 4), 5.0, device=DEV), torch.full((rows, H + 3), 5.0, device=DEV)
    ops.beam_gather([(a[:, :H], da[:, :H]), (b[:, 1:H], db[:, 1:H])], parent.to(DEV), W)
    torch.cuda.synchronize()
    idx = (torch.arange(rows) // W) * W + parent.long().clamp(0, W - 1)
    assert torch.equal(da[:, :H].cpu(), a.cpu()[idx, :H]) and torch.equal(db[:, 1:H].cpu(), b.cpu()[idx, 1:H])
    assert bool((da[:, H:] == 5.0).all()) and bool((db[:, H:] == 5.0).all()) and bool((db[:, 0] == 5.0).all())


@pytest.mark.parametrize("steps,B,W", [(1, 3, 2), (17, 5, 16)])
def test_beam_backtrack(steps, B, W):
    ops = _ops()
    rs = np.random.RandomState(steps)
    pa = torch.from_numpy(rs.randint(0, W, (steps, B, W)).astype(np.int32))
    tk = torch.from_numpy(rs.randint(0, 6, (steps, B, W)).astype(np.int32))
    sc = torch.from_numpy(rs.randn(steps, B, W).astype(np.float32))
    for eos in (1, -1):
        i32 = dict(dtype=torch.int32, device=DEV)
        tokens, beam, cum = torch.full((B, W, steps), -7, **i32), torch.full((B, W, steps), -7, **i32), torch.full((B, W, steps), 7.0, device=DEV)
        lens, final = torch.full((B, W), -7, **i32), torch.full((B, W), 7.0, device=DEV)
        ops.beam_backtrack(pa.to(DEV), tk.to(DEV), sc.to(DEV), eos, tokens, lens, final, beam_out=beam, cum_out=cum)
        torch.cuda.synchronize()
        ref = beam_check_backtrack(pa, tk, sc, eos, tokens, beam, cum, lens, final)
        assert eos < 0 or steps == 1 or ((ref["lens"] < steps).any() and (ref["lens"] == steps).any())
        tokens2, lens2, final2 = torch.zeros(B, W, steps, **i32), torch.zeros(B, W, **i32), torch.zeros(B, W, device=DEV)
        ops.beam_backtrack(pa.to(DEV), tk.to(DEV), sc.to(DEV), eos, tokens2, lens2, final2)
        assert torch.equal(tokens2, tokens) and torch.equal(lens2, lens) and torch.equal(final2, final)


def _same(a, b):
    """bit-identical results of two beam_decode(trace=True, want_logp=True) calls"""
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and torch.equal(x, y)
    for k in ("score", "parent", "token", "rows", "beam", "cum", "order"):
        assert torch.equal(a[4][k], b[4][k]), k


@pytest.mark.parametrize("weights,Bi,W,steps,arith", BEAM_CASES, ids=["%s-%dx%d" % c[:3] for c in BEAM_CASES])
def test_beam_decode_every_step_vs_the_definition_and_fp64_replay(weights, Bi, W, steps, arith):
    pkg = load_package()
    H, Z, sd = replay_inputs(weights)
    m = make_model(H, Z, sd, device=DEV, arith=arith)
    m.eval()
    eng = m.engine()
    x6 = bool(eng.ops.dw_x6 and eng.ops.cell_x6 and Bi * W >= eng.ops.cell_x6_rows and (Bi * W) % 128 == 0)
    assert x6 == (arith == "bf16x6")                       # the bf16 x 6 cells are the ones taken exactly where the case says so
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    rows = beam_rows(Bi)
    graphs = eng.__dict__.setdefault("_beam_graphs", {})

    def check(tag, z, res):
        tokens, scores, lens, logp, trace = (r if isinstance(r, dict) else r.cpu() for r in res)
        trace = {k: v.cpu() for k, v in trace.items()}
        assert not eng.ops.gru_sync_error()
        assert tokens.dtype == torch.int32 and tuple(tokens.shape) == (Bi, W, steps) and tuple(logp.shape) == (Bi, W, steps, V)
        beam_check_trace(trace, W, -1, tokens, scores, lens)
        assert bool((lens == steps).all())
        for j in sorted({0, W - 1}):
            st = beam_replay_check(sd, z, tokens[:, j], scores[:, j], logp[:, j], rows)
            print("\n" + beam_line("%s %s hypothesis %d" % (weights, tag, j), W, st), end="")

    z = replay_z(Bi, Z, Bi)
    zd = z.to(DEV)
    res = pkg.beam_decode(m, zd, steps, width=W, want_logp=True, trace=True)
    assert len(graphs) == 1
    check("graph", z, res)
    eager = pkg.beam_decode(m, zd, steps, width=W, want_logp=True, trace=True, use_graph=False)      # launch by launch: the same, bit for bit
    _same(res, eager)
    # another latent batch through the cached graph, then the first one again
    z2 = replay_z(Bi, Z, Bi + 1)
    res2 = pkg.beam_decode(m, z2.to(DEV), steps, width=W, want_logp=True, trace=True)
    assert len(graphs) == 1 and not torch.equal(res2[0], res[0])
    check("graph call 2", z2, res2)
    _same(res2, pkg.beam_decode(m, z2.to(DEV), steps, width=W, want_logp=True, trace=True, use_graph=False))
    _same(res, pkg.beam_decode(m, zd, steps, width=W, want_logp=True, trace=True))
    # the results without the log-probs: another graph, the same hypotheses
    t3, s3, l3 = pkg.beam_decode(m, zd, steps, width=W)
    assert len(graphs) == 2 and torch.equal(t3, res[0]) and torch.equal(s3, res[1]) and torch.equal(l3, res[2])
    # width 1 is a greedy stream of the same cells
    t1, s1, l1, lp1 = pkg.beam_decode(m, zd, steps, width=1, want_logp=True)
    assert len(graphs) == 3
    st = replay_decode_check(sd, z, t1[:, 0], lp1[:, 0], rows=rows)
    assert st["max_dlp"] <= st["tol_lp"]
    # eos = 1, and an eos the best hypotheses do write
    common = int(torch.mode(res[0][:, 0].reshape(-1))[0])
    for eos in (1, common):
        tokens, scores, lens, trace = pkg.beam_decode(m, zd, steps, width=W, eos=eos, trace=True)
        trace = {k: v.cpu() for k, v in trace.items()}
        ref = beam_check_trace(trace, W, eos, tokens.cpu(), scores.cpu(), lens.cpu())
        tk, ln = tokens.cpu().numpy(), lens.cpu().numpy()
        hit = tk == eos
        assert np.array_equal(ln, np.where(hit.any(2), hit.argmax(2) + 1, steps))
        after = np.arange(steps)[None, None, :] >= ln[:, :, None]
        assert (tk[after] == eos).all()
        cum = ref["cum"].view(np.uint32)
        frozen = np.arange(steps)[None, None, :] >= np.maximum(ln, 1)[:, :, None] - 1
        assert (np.where(frozen, cum, cum[np.arange(Bi)[:, None], np.arange(W)[None, :], ln - 1][:, :, None])
                == cum[np.arange(Bi)[:, None], np.arange(W)[None, :], ln - 1][:, :, None]).all()
        if eos == common:
            assert (ln < steps).any()
    assert len(graphs) == 4 and not eng.ops.gru_sync_error()
    print()


def test_the_other_decodes_are_untouched_by_beam_search():
    pkg = load_package()
    H, Z, sd = replay_inputs("h64")
    m = make_model(H, Z, sd, device=DEV)
    m.eval()
    eng = m.engine()
    zd = replay_z(17, Z, 3).to(DEV)

    def others():
        out = []
        for one in (True, False):                               # the one-launch kernel, then the per-token graph
            eng.single_launch_decode = one
            out.extend(pkg.greedy_decode(m, zd, 40))
        eng.single_launch_decode = True
        out.extend(pkg.sample_decode(m, zd, 40, temperature=1.1, seed=2))
        return out

    before = others()
    sizes = (len(eng._decode_graphs), len(eng._sample_graphs))
    tokens, scores, lens = pkg.beam_decode(m, zd, 40, width=4)
    assert len(eng._beam_graphs) == 1 and tuple(tokens.shape) == (17, 4, 40)
    from music_fader_nets_amd import decode as dec
    for w in range(1, dec.MAX_MASKED_GRAPHS + 3):               # every width captures a graph with static slabs of its own: the oldest goes
        pkg.beam_decode(m, zd, 8, width=w)
    assert len(eng._beam_graphs) == dec.MAX_MASKED_GRAPHS
    t2, s2, l2 = pkg.beam_decode(m, zd, 40, width=4)
    assert torch.equal(t2, tokens) and torch.equal(s2, scores) and torch.equal(l2, lens)
    for a, b in zip(before, others()):
        assert torch.equal(a, b)
    assert (len(eng._decode_graphs), len(eng._sample_graphs)) == sizes and not eng.ops.gru_sync_error()
