"""Constrained decode (decode.Constraints, fn_constrain_apply / fn_constrain_advance), CPU side: the two statements of the definition against each
other, the host twin in a stand-alone sanitizer build, every ValueError of Constraints, the argument answers of the entry points, and the three
decodes with constraints through a FakeOps stand-in - the fed stream against the automaton, with the unconstrained run as the witness that the
constraints had something to do."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import make_model, replay_inputs, replay_z
from helpers_constrain import (CASE_SHAPES, ConstrainFakeOps, assert_stream_valid, bias_bans, constrained_replay_check, constraint_params,
                               full_constraints, kernel_cases, params_bytes, python_advance, python_apply, prompt_tokens, reference_case,
                               same_result, stream_violations)
from mfn_import import ROOT, load_package

V = 342
IDS = ["%dx%d" % s for s in CASE_SHAPES]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the definition, stated twice
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,v", CASE_SHAPES, ids=IDS)
def test_the_two_statements_of_the_definition_agree(rows, v):
    seen = dict(stuck=0, free=0, fixed=0, banned=0, changed=0)
    for c in kernel_cases(rows, v):
        a = reference_case(c)
        b = reference_case(c, python_apply, python_advance)
        same_result(a, b, c["tag"])
        assert np.array_equal(a["logits"][:, v:], c["x"][:, v:])                         # the columns behind V are not the kernels' to touch
        assert a["tok"].min() >= 0 and a["tok"].max() < v or not c["fixup"]
        seen["stuck"] += int(a["stuck"].sum())
        seen["free"] += int((a["stuck"] == 0).sum())
        seen["fixed"] += int(a["fixed"].sum())
        seen["banned"] += int(((a["logits"][:, :v] == -np.inf) & (c["x"][:, :v] > -np.inf)).sum())
        seen["changed"] += 0 if c["held"] is None else int((a["held"] != c["held"]).any(1).sum())
        if c["tag"].startswith("stuck"):
            assert a["stuck"].any() and (rows == 1 or c["tag"] != "stuck by grammar" or not a["stuck"].all()), c["tag"]
            y = c["x"][:, :v] + c["bias"][None, :]
            assert np.array_equal(a["logits"][a["stuck"] == 1][:, :v], y[a["stuck"] == 1])   # a stuck row keeps y
        if c["tag"] == "not stuck at min_len":
            assert not a["stuck"].any()
    assert all(n > 0 for n in seen.values()), seen                                     # every branch of the definition was taken


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the host twin in a stand-alone sanitizer build
# ------------------------------------------------------------------------------------------------------------------------------
def test_host_twin_stand_alone_under_sanitizers(tmp_path):
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    src = os.path.join(ROOT, "music-fader-nets_amd", "csrc", "host", "constrain_check.cpp")
    exe = str(tmp_path / "constrain_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror", src, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    n = 0
    for rows, v in CASE_SHAPES:
        for c in kernel_cases(rows, v):
            bias_mode = 0 if c["bias"] is None else c["bias"].ndim
            with open(fin, "wb") as f:
                f.write(np.array([rows, v, c["ld"], c["step"], bias_mode, c["held"] is not None, c["fixup"], c["alias"]], dtype=np.int32).tobytes()
                        + params_bytes(c["p"]).tobytes() + c["x"].tobytes() + (b"" if c["bias"] is None else c["bias"].tobytes())
                        + (b"" if c["held"] is None else c["held"].tobytes()) + c["tok"].tobytes() + c["fb"].tobytes())
            p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (c["tag"], p.stdout[-1000:], p.stderr[-3000:])
            out = np.frombuffer(open(fout, "rb").read(), dtype=np.int32)
            assert out.size == 2 + rows * c["ld"] + 3 * rows + (4 * rows if c["held"] is not None else 0), (out.size, rows, v, c["tag"])
            o = [0]

            def take(k, dtype=np.int32, must_rc=False):
                if must_rc:
                    assert out[o[0]] == 0
                    o[0] += 1
                a = out[o[0]:o[0] + k].view(dtype)
                o[0] += k
                return a

            got = dict(logits=take(rows * c["ld"], np.float32, True).reshape(rows, c["ld"]), stuck=take(rows), tok=take(rows, must_rc=True),
                       held=None if c["held"] is None else take(rows * 4, np.uint32).reshape(rows, 4), fixed=take(rows))
            same_result(got, reference_case(c), "%dx%d %s" % (rows, v, c["tag"]))
            n += 1
    assert n >= 12 * 19


# ------------------------------------------------------------------------------------------------------------------------------
# 3. validation and the ABI without a GPU
# ------------------------------------------------------------------------------------------------------------------------------
def test_constraints_validation():
    pkg = load_package()
    Cn, EV = pkg.Constraints, pkg.EventVocab
    nan, inf = float("nan"), float("inf")
    good = torch.zeros(V)
    bad_bias = [torch.full((V,), -inf), torch.zeros(V - 1), torch.zeros(2, 3, V), torch.zeros(V, dtype=torch.int64), torch.zeros(0, V)]
    for t, val in ((0, nan), (5, inf)):
        b = good.clone()
        b[t] = val
        bad_bias.append(b)
    rows = torch.zeros(3, V)
    rows[1] = -inf                                                   # one row of a per-row bias keeps nothing
    bad_bias.append(rows)
    for b in bad_bias:
        with pytest.raises(ValueError):
            Cn(bias=b)
    for kw in (dict(ban=range(V)), dict(ban=[V]), dict(ban=[-1]), dict(ban=[1.5]), dict(bias=good, ban=list(range(V))),
               dict(min_length=-1), dict(min_length=2.0), dict(min_length=3), dict(min_length=True, eos=1), dict(eos=V), dict(eos=-1), dict(eos=1.0),
               dict(off_needs_on=1), dict(no_reonset="yes"), dict(want_stats=None), dict(max_polyphony=-1), dict(max_polyphony=129),
               dict(max_polyphony=2.0), dict(vocab=EV(2, 90, 129)), dict(vocab=EV(2, 90, -1)), dict(vocab=EV(-1, 90, 88)), dict(vocab=EV(300, 90, 88)),
               dict(vocab=EV(2, 300, 88)), dict(vocab=EV(2, 60, 88)), dict(vocab=EV(90, 2, 89)), dict(vocab=(2, 90)), dict(vocab=5),
               dict(vocab=EV(2, 90, 0), off_needs_on=True), dict(vocab=None, max_polyphony=2), dict(vocab=EV(2.0, 90, 88))):
        with pytest.raises(ValueError):
            Cn(**kw)
    c = Cn(bias=good, ban=(0, 7), min_length=4, eos=1, off_needs_on=True, max_polyphony=3)
    assert c.bias[0] == -inf and c.bias[7] == -inf and c.bias[1] == 0 and good[0] == 0 and c.stateful and c.key() == (1, True)
    assert constraint_params(c) == dict(on_lo=2, off_lo=90, n_pitch=88, max_poly=3, eos=1, min_len=4, flags=1)
    assert Cn().key() == (0, False) and Cn(ban=[3]).key() == (1, False) and Cn(bias=torch.zeros(4, V), no_reonset=True).key() == (2, True)
    assert Cn(vocab=EV(2, 90, 88)).vocab == (2, 90, 88) and "INFERRED" in Cn.__doc__ and "trainer_glsr.py:125,133" in Cn.__doc__


def test_entry_points_argument_errors_without_gpu():
    load_package()
    from music_fader_nets_amd import _lib
    lib = _lib.load()
    assert lib.fn_version() == 6 and C.sizeof(_lib.FnConstrainParams) == 32 and (_lib.CONSTRAIN_OFF_NEEDS_ON, _lib.CONSTRAIN_NO_REONSET) == (1, 2)
    buf, ibuf = (C.c_float * 4096)(), (C.c_int32 * 4096)()
    px, pi = C.cast(buf, C.c_void_p), C.cast(ibuf, C.c_void_p)

    def apply(logits=px, rows=2, v=V, ld=V, step=0, prm=pi, bias=None, rs=0, held=None, stuck=None):
        return lib.fn_constrain_apply(logits, rows, v, ld, step, prm, bias, rs, held, stuck, None)

    for kw in (dict(logits=None), dict(prm=None)):
        assert apply(**kw) == -1, kw
    for kw in (dict(rows=0), dict(v=0, ld=0), dict(v=1025, ld=1025), dict(ld=V - 1), dict(step=-1), dict(bias=px, rs=V - 1), dict(bias=px, rs=1),
               dict(bias=px, rs=-V)):
        assert apply(**kw) == -2, kw

    def advance(tok=pi, tld=1, rows=2, v=V, prm=pi, logits=None, ld=V, fb=None, fld=1, hin=None, hout=None, fixed=None):
        return lib.fn_constrain_advance(tok, tld, rows, v, prm, logits, ld, fb, fld, hin, hout, fixed, None)

    for kw in (dict(tok=None), dict(prm=None), dict(logits=px), dict(hin=pi)):
        assert advance(**kw) == -1, kw
    for kw in (dict(rows=0), dict(v=0), dict(v=1025), dict(tld=0), dict(logits=px, fb=pi, ld=V - 1), dict(logits=px, fb=pi, fld=0)):
        assert advance(**kw) == -2, kw
    hdr = open(os.path.join(ROOT, "include", "fadernets.h")).read()
    assert "FN_CONSTRAIN_OFF_NEEDS_ON 1" in hdr and "FN_CONSTRAIN_NO_REONSET 2" in hdr
    assert "fn_constrain_apply_host" in open(os.path.join(ROOT, "include", "fadernets_host.h")).read()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the three decodes through the stand-in
# ------------------------------------------------------------------------------------------------------------------------------
_WEIGHTS = {}
STEPS = 24


def _fake_model(cells=False):
    if "h64" not in _WEIGHTS:
        _WEIGHTS["h64"] = replay_inputs("h64")
    H, Z, sd = _WEIGHTS["h64"]
    m = make_model(H, Z, sd, ops=ConstrainFakeOps())
    m.eval()
    if cells:
        m.engine().cell_decode_rows = 1
    return m, sd, Z


def check_decode(con, fed, logp, stats, Bi):
    p = constraint_params(con)
    assert int(stats["stuck"].sum()) == 0
    return assert_stream_valid(fed, p, con.stateful, bias_bans(con, Bi), logp)


@pytest.mark.parametrize("mode", ["greedy", "sample"])
@pytest.mark.parametrize("cells", [False, True], ids=["scan_steps", "cells"])
def test_constrained_streams_on_the_cpu(mode, cells):
    pkg = load_package()
    m, sd, Z = _fake_model(cells)
    Bi = 5
    z = replay_z(Bi, Z, 11)
    con = full_constraints(pkg, per_row=Bi if cells else 0)
    prompt = prompt_tokens(Bi)
    if mode == "greedy":
        full = torch.zeros(Bi, STEPS, dtype=torch.int64)
        full[:, :3] = prompt
        run = lambda c: pkg.greedy_decode(m, z, STEPS, forced=full, force=3, constraints=c)          # noqa: E731
        fed_of = lambda tk: pkg.fed_tokens(tk, full, 3)                                                # noqa: E731
    else:
        run = lambda c: pkg.sample_decode(m, z, STEPS, temperature=1.3, seed=5, prompt=prompt, constraints=c)      # noqa: E731
        fed_of = lambda tk: tk                                                                          # noqa: E731
    logp, tokens, stats = run(con)
    fed = fed_of(tokens)
    st = check_decode(con, fed, logp, stats, Bi)
    assert st["note_ons"] > 3 * Bi and st["max_poly_seen"] == 3                         # the ceiling was reached, and held
    p = constraint_params(con)
    rep = constrained_replay_check(sd, z, fed, logp, p, True, con.bias, rows=np.arange(Bi), own=tokens if mode == "greedy" else None)
    assert rep["banned_share"] > 0.1
    if mode == "sample":
        assert int(stats["fixed"].sum()) == 0                                            # the fp32 restatement draws no zero-weight token here
    # the witness: without constraints the same call breaks every rule, and its stream is another one
    lp0, tk0 = run(None)
    v0 = stream_violations(fed_of(tk0), p, True, bias_bans(con, Bi))
    assert v0["banned"] > 0 and not torch.equal(tk0, tokens) and bool(torch.isfinite(lp0).all())
    # ... and with the bias alone (no grammar) the grammar is what breaks
    res = run(pkg.Constraints(bias=con.bias))
    assert len(res) == 2
    v1 = stream_violations(fed_of(res[1]), p, True, bias_bans(con, Bi))
    assert v1["banned"] > 0 and not torch.equal(res[1], tokens), v1


@pytest.mark.parametrize("Bi,W", [(2, 4), (3, 2)])
def test_constrained_beams_on_the_cpu(Bi, W):
    pkg = load_package()
    m, sd, Z = _fake_model(True)
    z = replay_z(Bi, Z, 21)
    con = full_constraints(pkg, per_row=Bi if W == 2 else 0)
    tokens, scores, lens, logp, stats = pkg.beam_decode(m, z, STEPS, width=W, eos=1, want_logp=True, constraints=con)
    assert tuple(tokens.shape) == (Bi, W, STEPS) and tuple(stats["stuck"].shape) == (Bi * W,) and int(stats["fixed"].sum()) == 0
    p = constraint_params(con)
    seen = 0
    for j in range(W):
        st = check_decode(con, tokens[:, j], logp[:, j], stats, Bi)
        seen = max(seen, st["max_poly_seen"])
        constrained_replay_check(sd, z, tokens[:, j], logp[:, j], p, True, con.bias, rows=np.arange(Bi), scores=scores[:, j] if bool((lens[:, j] == STEPS).all()) else None)
    assert seen == 3 and bool(torch.isfinite(scores).all())
    t0 = pkg.beam_decode(m, z, STEPS, width=W, eos=1)[0]
    v0 = sum(stream_violations(t0[:, j], p, True, bias_bans(con, Bi))["banned"] for j in range(W))
    assert v0 > 0 and not torch.equal(t0, tokens)
    with pytest.raises(ValueError):
        pkg.beam_decode(m, z, STEPS, width=W, eos=2, constraints=con)                 # the constraints' eos is the beam's
    with pytest.raises(ValueError):
        pkg.beam_decode(m, z, STEPS, width=W, constraints=con)


def test_fewer_allowed_continuations_than_beams_gives_minus_inf_scores():
    pkg = load_package()
    m, sd, Z = _fake_model(True)
    z = replay_z(2, Z, 4)
    bias = torch.full((V,), float("-inf"))
    bias[[200, 201]] = 0.0
    tokens, scores, lens = pkg.beam_decode(m, z, 1, width=4, constraints=pkg.Constraints(bias=bias))
    assert bool(torch.isfinite(scores[:, :2]).all()) and bool((scores[:, 2:] == float("-inf")).all())      # step 0 has two continuations for four beams
    assert set(tokens[:, :2].reshape(-1).tolist()) == {200, 201}
    tokens, scores, lens = pkg.beam_decode(m, z, 3, width=4, constraints=pkg.Constraints(bias=bias))       # two steps on there are four allowed streams
    assert bool(torch.isfinite(scores).all()) and set(tokens.reshape(-1).tolist()) == {200, 201}


def test_without_constraints_nothing_changes():
    pkg = load_package()
    m, sd, Z = _fake_model()
    ops = m.engine().ops
    z = replay_z(4, Z, 2)
    for cells in (False, True):
        m.engine().cell_decode_rows = 1 if cells else 10 ** 6
        del ops.calls[:]
        a = pkg.greedy_decode(m, z, 10)
        b = pkg.sample_decode(m, z, 10, seed=3)
        c = pkg.beam_decode(m, z, 10, width=3)
        assert not [x for x in ops.calls if x.startswith("constrain")]
        n_calls = len(ops.calls)
        # constraints that ban nothing: the same tokens and log-probs, two more calls per step at most
        none = pkg.Constraints()
        a2 = pkg.greedy_decode(m, z, 10, constraints=none)
        b2 = pkg.sample_decode(m, z, 10, seed=3, constraints=none)
        c2 = pkg.beam_decode(m, z, 10, width=3, constraints=none)
        for x, y in zip(a + b + c, a2 + b2 + c2):
            assert torch.equal(x, y)
        assert ops.calls.count("constrain_apply") == 30 and ops.calls.count("constrain_advance") == 10          # only the sampler's fix-up
        assert len(ops.calls) == 2 * n_calls + 40
    # stateful constraints: greedy advances every step, beams every step but the last
    del ops.calls[:]
    con = pkg.Constraints(no_reonset=True)
    pkg.greedy_decode(m, z, 10, constraints=con)
    assert ops.calls.count("constrain_advance") == 10
    pkg.beam_decode(m, z, 10, width=3, constraints=con)
    assert ops.calls.count("constrain_advance") == 19 and ops.calls.count("beam_gather") == 9


def test_fader_sweep_and_argument_errors():
    pkg = load_package()
    m, sd, Z = _fake_model()
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, V, (2, 12), generator=g)
    chroma = torch.rand(2, 24, generator=g)
    eps = (torch.randn(2, Z, generator=g), torch.randn(2, Z, generator=g))
    vals = [-1.0, 0.5, 2.0]
    con = full_constraints(pkg)
    p = constraint_params(con)
    for kw in (dict(), dict(sample=dict(seed=4)), dict(beam=dict(width=2, eos=1)), dict(prompt=torch.tensor([7, 11, 95]))):
        tok, _ = pkg.fader_sweep(m, x, chroma, vals, steps=16, eps=eps, constraints=con, **kw)
        assert tuple(tok.shape) == (2, 3, 16)
        assert_stream_valid(tok.reshape(6, 16), p, True, bias_bans(con, 6))
        plain, _ = pkg.fader_sweep(m, x, chroma, vals, steps=16, eps=eps, **kw)
        assert not torch.equal(plain, tok)
    z = replay_z(4, Z, 1)
    ops = m.engine().ops
    del ops.calls[:]
    for fn in (lambda c: pkg.greedy_decode(m, z, 8, constraints=c), lambda c: pkg.sample_decode(m, z, 8, constraints=c),
               lambda c: pkg.beam_decode(m, z, 8, constraints=c)):
        for c in ("off_needs_on", dict(ban=[0]), pkg.Constraints(bias=torch.zeros(3, V))):      # not a Constraints; a per-row bias of another batch
            with pytest.raises(ValueError):
                fn(c)
    assert ops.calls == []                                            # nothing was launched
