"""Beam-search decode (decode.beam_decode, fn_beam_step / fn_beam_gather / fn_beam_backtrack), CPU side: the two statements of the definition against
each other, the checkers against planted faults, beam_decode through a FakeOps stand-in on the inputs the GPU tests use (fp64 replay of the returned
hypotheses, the cap), the host twin in a stand-alone sanitizer build, the argument answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import make_model, replay_inputs, replay_z
from helpers_beam import (BEAM_CASES, STEP_SHAPES, BeamFakeOps, beam_check_backtrack, beam_check_gather, beam_check_step, beam_check_trace,
                          beam_line, beam_replay_check, beam_rows, python_beam_step, reference_backtrack, reference_beam_step, reference_gather,
                          step_inputs)
from mfn_import import ROOT, load_package

V = 342


def _lp(x, v):
    return torch.log_softmax(x[:, :v], dim=-1).numpy()


def _eos_of(v, want):
    return want if want < v else v - 1


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the definition, stated twice
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,W,v", STEP_SHAPES, ids=["%dx%dx%d" % s for s in STEP_SHAPES])
def test_the_two_statements_of_the_definition_agree(B, W, v):
    for step in (0, 5):
        for eos in (-1, _eos_of(v, 1)):
            x, sp, tp = step_inputs(B, W, v, step, eos, seed=B * 100 + W)
            lp = _lp(x, v)
            a = reference_beam_step(lp, W, step, eos, sp, tp)
            b = python_beam_step(lp, W, step, eos, sp, tp)
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (step, eos)
            assert not np.isnan(a[0]).any() and a[1].min() >= 0 and a[1].max() < W and a[2].min() >= 0 and a[2].max() < v
            if step == 0:
                assert (a[1] == 0).all()                              # only beam 0 is live
            elif eos >= 0 and W > 1:
                fin = tp.numpy() == eos
                took = fin[np.arange(B)[:, None], a[1]]
                assert fin.any() and (a[2][took] == eos).all()        # a finished beam is only ever continued by eos, at its own score
                assert np.array_equal(a[0][took].view(np.uint32), sp.numpy()[np.arange(B)[:, None], a[1]][took].view(np.uint32))
    # planted exact ties: sequence 0's rows are identical with equal previous scores and tokens 1 and v-1 tie at their top - the lower beam first, then the lower token
    if v >= 4:
        x, sp, tp = step_inputs(B, W, v, 5, -1, seed=7)
        s, p, t = reference_beam_step(_lp(x, v), W, 5, -1, sp, tp)
        assert t[0, 0] == 1 and p[0, 0] == 0
        if W >= 2:
            assert s[0, 0] == s[0, 1] and (p[0, 1], t[0, 1]) == (0, v - 1)
        if W >= 3:
            assert s[0, 0] == s[0, 2] and (p[0, 2], t[0, 2]) == (1, 1)
        x, sp, tp = step_inputs(B, W, v, 0, -1, seed=7)
        s, p, t = reference_beam_step(_lp(x, v), W, 0, -1)
        assert t[0, 0] == 1 and (W < 2 or (t[0, 1] == v - 1 and s[0, 1] == s[0, 0]))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the checkers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean():
    """a search of 4 sequences x 4 beams x 7 steps over 24 tokens with eos = 1 on random log-prob rows"""
    B, W, v, steps, eos = 4, 4, 24, 7, 1
    g = torch.Generator().manual_seed(5)
    sc, pa, tk = (np.zeros((steps, B, W), d) for d in (np.float32, np.int32, np.int32))
    rows = np.zeros((steps, B * W, v), np.float32)
    for i in range(steps):
        x = torch.randn(B * W, v, generator=g) * 2
        x[:, eos] += 1.5
        x.view(B, W, v)[0] = x.view(B, W, v)[0, 0].clone()            # sequence 0: identical rows whose two best tokens tie
        x.view(B, W, v)[0, :, 3] = x.view(B, W, v)[0, :, 7] = 6.0
        rows[i] = _lp(x, v)
        sc[i], pa[i], tk[i] = reference_beam_step(rows[i], W, i, eos, sc[i - 1] if i else None, tk[i - 1] if i else None)
    bt = reference_backtrack(pa, tk, sc, eos)
    trace = dict(score=sc, parent=pa, token=tk, rows=rows, beam=bt["beam"], cum=bt["cum"], order=np.broadcast_to(np.arange(W), (B, W)))
    return trace, W, eos, bt


def test_checkers_accept_the_restatement(clean):
    trace, W, eos, bt = clean
    ref = beam_check_trace(trace, W, eos, bt["tokens"], bt["final"], bt["lens"])
    assert (ref["lens"] < 7).any() and (ref["lens"] == 7).any()
    fin = trace["token"][:-1] == eos
    assert fin.any() and not fin.all()


def _step_args(trace, i):
    return (trace["rows"][i], trace["score"][i - 1], trace["token"][i - 1], trace["score"][i].copy(), trace["parent"][i].copy(), trace["token"][i].copy())


def test_checkers_reject_planted_faults(clean):
    trace, W, eos, bt = clean
    steps = trace["score"].shape[0]
    # a wrong tie order: two outputs of equal score swapped
    hit = None
    for i in range(1, steps):
        s = trace["score"][i]
        for b, j in np.argwhere(s[:, :-1] == s[:, 1:]):
            hit = hit or (i, int(b), int(j))
    assert hit is not None
    i, b, j = hit
    rows, sp, tp, s, p, t = _step_args(trace, i)
    p[b, [j, j + 1]], t[b, [j, j + 1]] = p[b, [j + 1, j]], t[b, [j + 1, j]]
    with pytest.raises(AssertionError, match=r"\(sel\)"):
        beam_check_step(rows, W, i, eos, sp, tp, s, p, t)
    # a finished beam that was extended: the step taken as if there were no eos
    i = next(i for i in range(1, steps) if (trace["token"][i - 1] == eos).any())
    rows, sp, tp, s, p, t = _step_args(trace, i)
    ext = reference_beam_step(rows, W, i, -1, sp, tp)
    assert not np.array_equal(ext[2], t) or not np.array_equal(ext[1], p)
    with pytest.raises(AssertionError, match=r"\((sel|score)\)"):
        beam_check_step(rows, W, i, eos, sp, tp, *ext)
    # a parent off by one
    rows, sp, tp, s, p, t = _step_args(trace, 3)
    p[2, 1] = (p[2, 1] + 1) % W
    with pytest.raises(AssertionError, match=r"\(sel\)"):
        beam_check_step(rows, W, 3, eos, sp, tp, s, p, t)
    # a score that is not the one fp32 add
    rows, sp, tp, s, p, t = _step_args(trace, 3)
    s[1, 2] = np.nextafter(s[1, 2], np.float32(0))
    with pytest.raises(AssertionError, match=r"\(score\)"):
        beam_check_step(rows, W, 3, eos, sp, tp, s, p, t)
    # a gather that ignored parent
    src = np.random.RandomState(0).rand(trace["parent"][3].size, 12).astype(np.float32)
    par = trace["parent"][3].reshape(-1)
    assert (par != np.arange(par.size) % W).any()
    beam_check_gather(reference_gather(src, par, W), src, par, W)
    with pytest.raises(AssertionError, match=r"\(gather\)"):
        beam_check_gather(src.copy(), src, par, W)
    # ... and one that indexed the whole batch instead of the sequence's own beams
    with pytest.raises(AssertionError, match=r"\(gather\)"):
        beam_check_gather(src[np.clip(par, 0, W - 1)], src, par, W)
    # a backtrack off by one step: the tokens read with the parent already applied
    sc, pa, tk = trace["score"], trace["parent"], trace["token"]
    bad = np.zeros_like(bt["tokens"])
    cur = np.broadcast_to(np.arange(W), pa.shape[1:]).copy()
    bb = np.arange(pa.shape[1])[:, None]
    for i in range(steps - 1, -1, -1):
        cur = pa[i][bb, cur]
        bad[:, :, i] = tk[i][bb, cur]
    with pytest.raises(AssertionError, match=r"\(backtrack\)"):
        beam_check_backtrack(pa, tk, sc, eos, bad, None, None, None, None)
    with pytest.raises(AssertionError, match=r"\(backtrack\)"):
        beam_check_backtrack(pa, tk, sc, eos, None, None, None, bt["lens"] - 1, None)
    with pytest.raises(AssertionError, match=r"\(backtrack\)"):
        beam_check_trace(trace, W, eos, np.roll(bt["tokens"], 1, axis=2))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. beam_decode through the stand-in
# ------------------------------------------------------------------------------------------------------------------------------
_WEIGHTS = {}


def _fake_model(weights="h64"):
    if weights not in _WEIGHTS:
        _WEIGHTS[weights] = replay_inputs(weights)
    H, Z, sd = _WEIGHTS[weights]
    m = make_model(H, Z, sd, ops=BeamFakeOps())
    m.eval()
    m.engine().cell_decode_rows = 1          # the greedy decode on the cells too: the same stand-in arithmetic as the beam loop's
    return m, sd, Z


@pytest.mark.parametrize("weights,Bi,W,steps,arith", BEAM_CASES, ids=["%s-%dx%d" % c[:3] for c in BEAM_CASES])
def test_beam_decode_on_the_cpu(weights, Bi, W, steps, arith):
    """the replayed rows of a GPU case, decoded by the stand-in: every step's slabs, the backtrack, and every returned hypothesis against the fp64
    replay of its own tokens - rules (a) - (c), the score sum and the cap of the positions whose fp64 top-2 gap is below delta"""
    pkg = load_package()
    m, sd, Z = _fake_model(weights)
    rows = beam_rows(Bi)
    z = replay_z(Bi, Z, Bi)[rows]
    tokens, scores, lens, logp, trace = pkg.beam_decode(m, z, steps, width=W, want_logp=True, trace=True)
    n = len(rows)
    assert tokens.dtype == torch.int32 and tuple(tokens.shape) == (n, W, steps) and tuple(scores.shape) == (n, W) and tuple(lens.shape) == (n, W)
    assert tuple(logp.shape) == (n, W, steps, V) and bool((lens == steps).all())
    beam_check_trace(trace, W, -1, tokens, scores, lens)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    for j in range(W):
        st = beam_replay_check(sd, z, tokens[:, j], scores[:, j], logp[:, j], np.arange(n))
        print("\n" + beam_line("stand-in %s hypothesis %d" % (weights, j), W, st), end="")
    # the W hypotheses of a sequence are distinct streams
    for b in range(n):
        assert len({tuple(tokens[b, j].tolist()) for j in range(W)}) == W


def test_beam_decode_width_one_is_the_greedy_decode():
    pkg = load_package()
    m, sd, Z = _fake_model()
    z = replay_z(6, Z, 13)
    lpg, tkg = pkg.greedy_decode(m, z, 40)
    tokens, scores, lens, logp = pkg.beam_decode(m, z, 40, width=1, want_logp=True)
    assert torch.equal(tokens[:, 0], tkg) and torch.equal(logp[:, 0], lpg)
    assert bool((lens == 40).all()) and tuple(scores.shape) == (6, 1)


def test_beam_decode_eos_and_length_penalty():
    pkg = load_package()
    m, sd, Z = _fake_model()
    z = replay_z(6, Z, 3)
    steps, W = 30, 4
    t0 = pkg.beam_decode(m, z, steps, width=W, trace=True)
    eos = int(torch.mode(t0[0][:, 0, 4:12].reshape(-1))[0])           # a token the best hypotheses do write
    tokens, scores, lens, trace = pkg.beam_decode(m, z, steps, width=W, eos=eos, trace=True)
    ref = beam_check_trace(trace, W, eos, tokens, scores, lens)
    assert bool((lens < steps).any())
    tk, ln = tokens.numpy(), lens.numpy()
    for b in range(tk.shape[0]):
        for j in range(W):
            L = ln[b, j]
            assert (tk[b, j, :L - 1] != eos).all() and (L == steps or (tk[b, j, L - 1:] == eos).all())
            if L < steps:                                                # frozen: the cumulative score stays from the end on
                assert len(set(ref["cum"][b, j, L - 1:].view(np.uint32).tolist())) == 1
    # a length penalty re-sorts the same hypotheses, stably
    tp, sp, lp_, tr = pkg.beam_decode(m, z, steps, width=W, eos=eos, length_penalty=1.0, trace=True)
    order = tr["order"].numpy()
    key = scores.numpy() / ln.astype(np.float32) ** np.float32(1.0)
    assert np.array_equal(order, np.argsort(-key, axis=1, kind="stable")) and (order != np.arange(W)).any()
    bb = np.arange(tk.shape[0])[:, None]
    assert np.array_equal(tp.numpy(), tk[bb, order]) and np.array_equal(sp.numpy(), scores.numpy()[bb, order]) and np.array_equal(lp_.numpy(), ln[bb, order])


def test_beam_decode_leaves_the_other_decodes_alone():
    pkg = load_package()
    m, sd, Z = _fake_model()
    ops = m.engine().ops
    z = replay_z(4, Z, 2)
    pkg.greedy_decode(m, z, 10)
    assert not [c for c in ops.calls if c.startswith("beam")]
    seen = []
    ops.vocab_argmax = lambda *a, **k: seen.append("vocab_argmax")
    ops.out_argmax = lambda *a, **k: seen.append("out_argmax")
    ops.gru_seq_fwd = lambda *a, **k: seen.append("gru_seq_fwd")
    del ops.calls[:]
    pkg.beam_decode(m, z, 10, width=3)
    assert ops.calls.count("beam_step") == 10 and ops.calls.count("beam_gather") == 9 and ops.calls.count("beam_backtrack") == 1 and not seen
    assert ops.calls.count("gemm") == 2 + 10


def test_fader_sweep_beam():
    pkg = load_package()
    m, sd, Z = _fake_model()
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, V, (2, 12), generator=g)
    chroma = torch.rand(2, 24, generator=g)
    eps = (torch.randn(2, Z, generator=g), torch.randn(2, Z, generator=g))
    vals = [-1.0, 0.5, 2.0]
    plain, z0 = pkg.fader_sweep(m, x, chroma, vals, steps=16, eps=eps)
    one, z1 = pkg.fader_sweep(m, x, chroma, vals, steps=16, eps=eps, beam=dict(width=1))
    assert tuple(one.shape) == (2, 3, 16) and one.dtype == torch.int32 and torch.equal(z0, z1) and torch.equal(one, plain)
    four, _ = pkg.fader_sweep(m, x, chroma, vals, steps=16, eps=eps, beam=dict(width=4, eos=1, length_penalty=0.5))
    assert tuple(four.shape) == (2, 3, 16)
    for kw in (dict(beam=dict(width=2), sample=dict(seed=1)), dict(beam=dict(width=2), prompt=torch.tensor([5, 7])), dict(beam=dict(wdith=2)),
               dict(beam=dict(width=0)), dict(beam=dict(width=17)), dict(beam=dict(eos=V)), dict(beam=dict(length_penalty=float("nan")))):
        with pytest.raises(ValueError):
            pkg.fader_sweep(m, x, chroma, vals, steps=16, eps=eps, **kw)


def test_beam_decode_argument_errors():
    pkg = load_package()
    m, sd, Z = _fake_model()
    z = replay_z(4, Z, 1)
    ops = m.engine().ops
    calls = []
    for name in ("gemm", "gru_cell", "beam_step", "beam_gather", "beam_backtrack"):       # nothing may be launched before the arguments are accepted
        orig = getattr(ops, name)
        setattr(ops, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    for kw in (dict(width=0), dict(width=17), dict(width=-1), dict(width=2.0), dict(width=True), dict(width=None), dict(eos=-1), dict(eos=V), dict(eos=1.0),
               dict(eos=True), dict(length_penalty=float("inf")), dict(length_penalty=float("nan")), dict(length_penalty="1"), dict(length_penalty=None)):
        with pytest.raises(ValueError):
            pkg.beam_decode(m, z, 20, **kw)
    for steps in (0, -3, 2.5, None):
        with pytest.raises(ValueError):
            pkg.beam_decode(m, z, steps)
    assert calls == []
    pkg.beam_decode(m, z, 3, width=16, eos=V - 1, length_penalty=-0.5)
    assert "beam_step" in calls and "gemm" in calls


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the host twin in a stand-alone sanitizer build, 5. the ABI without a GPU
# ------------------------------------------------------------------------------------------------------------------------------
def test_host_twin_stand_alone_under_sanitizers(tmp_path):
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    src = os.path.join(ROOT, "music-fader-nets_amd", "csrc", "host", "beam_check.cpp")
    exe = str(tmp_path / "beam_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror", src, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for n, (B, W, v) in enumerate(STEP_SHAPES):
        for step, eos in ((0, -1), (5, -1), (5, _eos_of(v, 1))):
            ld, cols, steps = v + (2 if v == V else 0), 5 + n, 1 + 3 * n
            x, sp, tp = step_inputs(B, W, v, step, eos, seed=50 + n, ld=ld)
            rs = np.random.RandomState(n)
            state = rs.rand(B * W, cols).astype(np.float32)
            pa, tk = rs.randint(0, W, (steps, B, W)).astype(np.int32), rs.randint(0, v, (steps, B, W)).astype(np.int32)
            sc = rs.randn(steps, B, W).astype(np.float32)
            with open(fin, "wb") as f:
                f.write(np.array([B, W, v, ld, step, eos, cols, steps], dtype=np.int32).tobytes() + x.numpy().tobytes() + sp.numpy().tobytes()
                        + tp.numpy().tobytes() + state.tobytes() + pa.tobytes() + tk.tobytes() + sc.tobytes())
            p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
            out = np.frombuffer(open(fout, "rb").read(), dtype=np.int32)
            R = B * W
            assert out.size == 3 + R * (3 + v + cols + 3 * steps + 2), (out.size, B, W, v)
            o = [0]

            def take(k, dtype=np.int32, must_rc=True):
                if must_rc:
                    assert out[o[0]] == 0
                    o[0] += 1
                a = out[o[0]:o[0] + k].view(dtype)
                o[0] += k
                return a

            score, parent, token, lp = take(R, np.float32), take(R, must_rc=False), take(R, must_rc=False), take(R * v, np.float32, False).reshape(R, v)
            good = ~np.isnan(x[:, :v].numpy()).any(1)
            assert np.abs(lp[good] - _lp(x, v)[good]).max() < 1e-4 and np.isnan(lp[~good]).all()
            beam_check_step(lp, W, step, eos, sp, tp, score, parent, token)              # bit for bit on the twin's own log-prob rows
            beam_check_gather(take(R * cols, np.float32).reshape(R, cols), state, parent, W)
            beam_check_backtrack(pa, tk, sc, eos, take(R * steps).reshape(B, W, steps), take(R * steps, must_rc=False).reshape(B, W, steps),
                                 take(R * steps, np.float32, False).reshape(B, W, steps), take(R, must_rc=False).reshape(B, W),
                                 take(R, np.float32, False).reshape(B, W))


def test_beam_entry_points_argument_errors_without_gpu():
    load_package()
    from music_fader_nets_amd import _lib
    lib = _lib.load()
    assert lib.fn_version() == 6 and _lib.FN_BEAM_MAX_W == 16 and C.sizeof(_lib.FnBeamGatherJob) == 32
    buf = (C.c_float * 4096)()
    ibuf = (C.c_int32 * 4096)()
    px, pi = C.cast(buf, C.c_void_p), C.cast(ibuf, C.c_void_p)

    def step(logits=px, B=1, W=4, v=V, ld=V, st=1, eos=-1, sprev=px, tprev=pi, pld=4, sc=px, pa=pi, tk=pi, old=4):
        return lib.fn_beam_step(logits, B, W, v, ld, st, eos, sprev, tprev, pld, sc, pa, tk, old, None, 0, None)

    for kw in (dict(logits=None), dict(sc=None), dict(pa=None), dict(tk=None), dict(sprev=None), dict(tprev=None)):
        assert step(**kw) == -1, kw
    for kw in (dict(B=0), dict(W=0), dict(W=17), dict(W=5, v=4, ld=4), dict(v=0, ld=0, W=1), dict(v=1025, ld=1025), dict(ld=V - 1), dict(st=-1), dict(eos=V),
               dict(eos=-2), dict(old=3), dict(pld=3)):
        assert step(**kw) == -2, kw
    job = (_lib.FnBeamGatherJob * 5)()
    for j in job:
        j.src, j.src_ld, j.dst, j.dst_ld, j.cols = px.value, 8, px.value + 4096, 8, 8

    def gather(jobs=job, n=1, rows=8, W=4, parent=pi):
        return lib.fn_beam_gather(jobs, n, rows, W, parent, None)

    assert gather(jobs=None) == -1 and gather(parent=None) == -1 and gather(n=0) == -5 and gather(n=5) == -5
    assert gather(rows=0) == -2 and gather(rows=7) == -2 and gather(W=17, rows=17) == -2 and gather(W=0) == -2
    job[0].dst = px.value
    assert gather() == -2                                               # dst == src
    job[0].dst, job[0].cols = px.value + 4096, 9
    assert gather() == -2
    job[0].cols, job[0].src = 8, None
    assert gather() == -1

    def back(pa=pi, tk=pi, sc=px, steps=2, B=1, W=4, eos=-1, tout=pi, lout=pi, sout=px):
        return lib.fn_beam_backtrack(pa, tk, sc, steps, B, W, eos, tout, None, None, lout, sout, None)

    for kw in (dict(pa=None), dict(tk=None), dict(sc=None), dict(tout=None), dict(lout=None), dict(sout=None)):
        assert back(**kw) == -1, kw
    for kw in (dict(steps=0), dict(B=0), dict(W=0), dict(W=17), dict(eos=-2)):
        assert back(**kw) == -2, kw
    hdr = open(os.path.join(ROOT, "include", "fadernets.h")).read()
    assert "gmm_model.py:73-80,119-149" in hdr and "fn_beam" not in open(os.path.join(ROOT, "include", "fadernets_host.h")).read()
