"""Seeded temperature / top-k / top-p sampling on a real MI355X: fn_vocab_sample alone (uniforms bit-equal to numpy, log-probs and argmax
bit-equal to fn_vocab_argmax, tokens against the fp64 definition), decode.sample_decode on the per-token paths (every step against an fp64
replay of the sampled stream and against the definition; cached graph, no graph, top_k = 1 = greedy, a prompt), and the greedy decode untouched."""
import numpy as np
import pytest
import torch

from helpers import make_model, replay_inputs, replay_rows, replay_z
from helpers_forced import forced_line, forced_tokens, replay_forced_check
from helpers_sampling import PARAMS_DTYPE, SETTINGS, sample_check, sample_check_decode, sample_line, sample_uniforms
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = 342


def _params_dev(s, seed, offset):
    raw = np.zeros(1, dtype=PARAMS_DTYPE)
    raw["seed"], raw["offset"], raw["inv_t"], raw["top_p"], raw["top_k"] = seed, offset, np.float32(1.0) / np.float32(s[0]), s[2], s[1]
    return torch.from_numpy(raw.view(np.uint8).copy()).to(DEV)


@pytest.mark.parametrize("B,V", [(9, 342), (1, 342), (5, 1024), (6, 385), (3, 65), (2, 1)])
def test_vocab_sample_kernel_alone(B, V):
    """three workgroups, the last with one live row (B = 9), and a single row, at the decoder's V = 342; the 16-entries-per-lane instance at its
    ends (V = 385, 1024), two entries per lane with a ragged last block (65), one entry in all (1); the outputs are strided columns / slices of
    larger matrices whose other entries must stay as they were"""
    load_package()
    from music_fader_nets_amd.engine import LOGIT_LD
    from music_fader_nets_amd.hipops import HipOps
    ops = HipOps(DEV)
    x = torch.zeros(B, LOGIT_LD if V == 342 else V + 3)
    x[:, :V] = torch.randn(B, V, generator=torch.Generator().manual_seed(40 + B)) * 8
    x[:, V:] = 1e9                                                  # the padding columns are no logits
    xd = x.to(DEV)
    lp_ref = torch.full((B, 3, V), 7.0, device=DEV)
    tk_ref = torch.full((B, 4), -5, dtype=torch.int32, device=DEV)
    ops.vocab_argmax(xd, V, lp_ref[:, 1, :], tk_ref[:, 2])
    for n, s in enumerate(SETTINGS):
        for step in (0, 5):
            seed, offset = (9 << 32) + n, (1 << 34) + step
            lp = torch.full((B, 3, V), 7.0, device=DEV)
            tok = torch.full((B, 4), -5, dtype=torch.int32, device=DEV)
            own = torch.full((B, 4), -5, dtype=torch.int32, device=DEV)
            u = torch.full((B + 1,), 7.0, device=DEV)
            ops.vocab_sample(xd, V, _params_dev(s, seed, offset), step, lp[:, 1, :], tok[:, step % 4], own_out=own[:, 2], u_out=u[:B])
            torch.cuda.synchronize()
            assert torch.equal(lp, lp_ref) and torch.equal(own, tk_ref)            # bit for bit, and nothing beside the strided views written
            assert float(u[B]) == 7.0 and int((tok == -5).sum()) == 3 * B
            un = sample_uniforms(np.arange(B), [step], seed, offset)[:, 0]
            assert np.array_equal(u[:B].cpu().numpy().view(np.uint32), un.view(np.uint32))
            st = sample_check(lp[:, 1, :].cpu().numpy(), tok[:, step % 4].cpu().numpy(), un, dict(T=s[0], k=s[1], p=s[2]))
            print("\n" + sample_line("kernel B %d step %d" % (B, step), dict(T=s[0], k=s[1], p=s[2]), st), end="")
            # the optional outputs left out: the same tokens
            tok2 = torch.zeros(B, dtype=torch.int32, device=DEV)
            ops.vocab_sample(xd, V, _params_dev(s, seed, offset), step, None, tok2)
            assert torch.equal(tok2, tok[:, step % 4])


SAMPLE_CASES = [("scan_steps", "h64", 17, 64), ("cells_f32", "h512", 705, 32), ("cells_x6", "h512", 2048, 24)]


@pytest.mark.parametrize("path,weights,Bi,steps", SAMPLE_CASES, ids=["%s-%s-%d" % (p, w, b) for p, w, b, _ in SAMPLE_CASES])
def test_sample_decode_paths_every_step_vs_fp64_replay(path, weights, Bi, steps):
    pkg = load_package()
    H, Z, sd = replay_inputs(weights)
    m = make_model(H, Z, sd, device=DEV, arith="bf16x6" if path == "cells_x6" else None)
    m.eval()
    eng = m.engine()
    eng.single_launch_decode = False
    from music_fader_nets_amd import decode as dec
    sampling = torch.zeros(32, dtype=torch.uint8)             # decode_path asks whether there are sampling parameters, not what they hold
    if path == "scan_steps":
        eng.cell_decode_rows = 1 << 30
        assert dec.decode_path(eng, Bi, True, sampling, None) == "scan_steps"
    else:
        assert dec.decode_path(eng, Bi, True, sampling, None) == "cells" and dec.decode_path(eng, Bi, False, sampling, None) == "cells"
        x6 = eng.ops.dw_x6 and eng.ops.cell_x6 and Bi >= eng.ops.cell_x6_rows
        assert x6 == (path == "cells_x6")
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    z = replay_z(Bi, Z, Bi)
    zd = z.to(DEV)
    rows = replay_rows(Bi)
    graphs = eng.__dict__.setdefault("_sample_graphs", {})
    all_forced = np.ones(steps, dtype=bool)

    def check(tag, lp, tk, par, P=0):
        assert not eng.ops.gru_sync_error()
        assert tk.dtype == torch.int32 and tuple(tk.shape) == (Bi, steps) and tuple(lp.shape) == (Bi, steps, V)
        own = torch.from_numpy(np.argmax(lp.cpu().numpy(), axis=-1))                       # first index of the maximum
        st = replay_forced_check(sd, z, own, tk, all_forced, tk, lp, rows=rows)
        print("\n" + forced_line("%s/%s %s" % (path, weights, tag), "sampled", H, st), end="")
        st = sample_check_decode(lp[rows], tk[rows], rows, par, P=P)
        print("\n" + sample_line("%s/%s %s" % (path, weights, tag), par, st), end="")

    for n, s in enumerate((SETTINGS[0], SETTINGS[4])):
        par = dict(T=s[0], k=s[1], p=s[2], seed=(Bi << 32) + n, offset=(1 << 32) + 7 * n)
        kw = dict(temperature=s[0], top_k=s[1], top_p=s[2], seed=par["seed"], offset=par["offset"])
        lp, tk = pkg.sample_decode(m, zd, steps, **kw)
        assert len(graphs) == 1
        check("setting %d" % n, lp, tk, par)
        lpn, tkn = pkg.sample_decode(m, zd, steps, use_graph=False, **kw)                  # launch by launch: the same, bit for bit
        assert torch.equal(tkn, tk) and torch.equal(lpn, lp)
        _, tko = pkg.sample_decode(m, zd, steps, want_logp=False, use_graph=False, **kw)
        assert torch.equal(tko, tk)
    # another seed and temperature on another latent batch: the cached graph
    z, par = replay_z(Bi, Z, Bi + 1), dict(T=1.3, k=40, p=0.95, seed=12345, offset=0)
    zd = z.to(DEV)
    lp, tk = pkg.sample_decode(m, zd, steps, temperature=1.3, top_k=40, top_p=0.95, seed=12345)
    assert len(graphs) == 1
    check("graph call 2", lp, tk, par)
    # top_k = 1 is the greedy decode of the same path
    lpg, tkg = pkg.greedy_decode(m, zd, steps)
    lp1, tk1 = pkg.sample_decode(m, zd, steps, temperature=0.5, top_k=1, top_p=0.3, seed=77)
    assert len(graphs) == 1 and torch.equal(tk1, tkg) and torch.equal(lp1, lpg)
    # a prompt
    P = steps // 3
    prompt = forced_tokens(Bi, P, Bi)
    lp, tk = pkg.sample_decode(m, zd, steps, temperature=0.8, top_k=40, top_p=0.95, seed=5, offset=9, prompt=prompt)
    assert len(graphs) == 2 and torch.equal(tk[:, :P].cpu().long(), prompt)
    check("prompt", lp, tk, dict(T=0.8, k=40, p=0.95, seed=5, offset=9), P=P)
    print()


def test_greedy_decode_is_untouched_by_sampling():
    pkg = load_package()
    H, Z, sd = replay_inputs("h64")
    m = make_model(H, Z, sd, device=DEV)
    m.eval()
    eng = m.engine()
    zd = replay_z(17, Z, 3).to(DEV)
    before = []
    for one in (True, False):                                   # the one-launch kernel, then the per-token graph
        eng.single_launch_decode = one
        before.append(pkg.greedy_decode(m, zd, 40))
    n = len(eng.__dict__.get("_decode_graphs", {}))
    assert n == 1
    eng.single_launch_decode = True                             # sampling takes the per-token launches whatever the greedy dispatch is
    lp, tk = pkg.sample_decode(m, zd, 40, temperature=1.1, seed=2)
    assert not torch.equal(tk, before[0][1]) and len(eng._sample_graphs) == 1 and len(eng._decode_graphs) == n
    # every prompt length captures a graph with static buffers of its own: at most MAX_MASKED_GRAPHS of them stay, the unprompted one with them
    from music_fader_nets_amd import decode as dec
    for P in range(1, dec.MAX_MASKED_GRAPHS + 3):
        pkg.sample_decode(m, zd, 40, seed=2, prompt=forced_tokens(17, P, 1))
    assert sum(1 for k in eng._sample_graphs if k[3]) == dec.MAX_MASKED_GRAPHS and sum(1 for k in eng._sample_graphs if not k[3]) == 1
    lp2, tk2 = pkg.sample_decode(m, zd, 40, temperature=1.1, seed=2)
    assert torch.equal(tk2, tk) and torch.equal(lp2, lp) and len(eng._decode_graphs) == n
    assert not eng.ops.gru_sync_error()
    for one, (lp0, tk0) in zip((True, False), before):
        eng.single_launch_decode = one
        lp1, tk1 = pkg.greedy_decode(m, zd, 40)
        assert torch.equal(tk1, tk0) and torch.equal(lp1, lp0)
    assert len(eng._decode_graphs) == n
