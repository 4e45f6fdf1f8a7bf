"""Forced-token feedback in decode (greedy_decode(..., forced, force), continue_from, fader_sweep(prompt=), fn_decode_forced), CPU side:
the replay checker of forced streams against planted faults, the per-token paths through FakeOps, the host twin under ASAN, the ABI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fake_ops import FakeOps
from helpers import REPLAY_CAP, make_model, replay_inputs, replay_line, replay_z
from helpers_forced import (FORCED_CASES, FORCED_GRAPH_PATHS, FORCED_MASKS, fed_stream, forced_line, forced_mask, forced_tokens,
                            oracle_forced_decode, replay_forced_check)
from mfn_import import ROOT, load_package
from oracle import gmvae_oracle as orc


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the checker
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean():
    """the fp32 oracle's forced decode (Bernoulli(0.5) mask, random forced tokens) of 24 rows x 300 steps on the seeded H = 64 inputs"""
    H, Z, sd = replay_inputs("h64")
    z = replay_z(24, Z, 5)
    forced, force = forced_tokens(24, 300, 5), forced_mask("bernoulli", 300, 5)
    lp, tk = oracle_forced_decode(sd, z, 300, forced, force)
    fed = fed_stream(tk, forced, force)
    st = replay_forced_check(sd, z, tk, forced, force, fed, lp)
    return sd, z, tk, lp, forced, force, fed, st


def test_forced_replay_accepts_the_clean_decode(clean):
    sd, z, tk, lp, forced, force, fed, st = clean
    assert st["rows"] == 24 and st["positions"] == 24 * 300 and 0.4 < st["forced_share"] < 0.6
    assert st["ratio"] == pytest.approx(1.0)                     # the stand-in IS the fp32 restatement
    assert 0 < st["e_ref"] and st["tol_lp"] == min(1e-4, 16 * st["e_ref"]) and st["delta"] == 2 * st["tol_lp"]
    assert not torch.equal(fed, tk) and not torch.equal(fed, forced)
    st2 = replay_forced_check(sd, z, tk, forced, force, fed)      # tokens only
    assert st2["share_below_delta"] == st["share_below_delta"]


def test_forced_oracle_ends_are_the_two_known_decoders():
    """all forced = the teacher-forced oracle decoder, none forced = the greedy one (bit for bit: the same arithmetic)"""
    H, Z, sd = replay_inputs("h64")
    z = replay_z(5, Z, 3)
    forced = forced_tokens(5, 40, 3)
    lp, _ = oracle_forced_decode(sd, z, 40, forced, forced_mask("all", 40))
    assert torch.equal(lp, orc.global_decoder(sd, z, 40, teacher=forced))
    lp, tk = oracle_forced_decode(sd, z, 40, forced, forced_mask("none", 40))
    lpg, tkg = orc.greedy_decode(sd, z, 40)
    assert torch.equal(lp, lpg) and torch.equal(tk, tkg)


def test_forced_replay_rejects_one_wrong_fed_entry(clean):
    """one entry of the reported fed stream at a late step replaced: at a forced step (not the forced token) and at a free one (not the own)"""
    sd, z, tk, lp, forced, force, fed, st = clean
    for s in (int(np.nonzero(force[:290])[0][-1]), int(np.nonzero(~force[:290])[0][-1])):
        assert s >= 250
        bad = fed.clone()
        bad[11, s] = (fed[11, s] + 1) % orc.E
        with pytest.raises(AssertionError, match=r"\(fed\)"):
            replay_forced_check(sd, z, tk, forced, force, bad, lp)


def test_forced_replay_rejects_an_argmax_fed_at_a_forced_step(clean):
    """a decoder that fed its own argmax at ONE forced step (step 260; the forced token there is not the argmax in the rows checked):
    everything it computed afterwards belongs to another stream than where(force, forced, tokens)"""
    sd, z, tk, lp, forced, force, fed, st = clean
    s = int(np.nonzero(force[:270])[0][-1])
    assert s >= 250
    lazy = force.copy()
    lazy[s] = False
    lp2, tk2 = oracle_forced_decode(sd, z, 300, forced, lazy)
    assert bool((tk2[:, s] != forced[:, s]).any())
    with pytest.raises(AssertionError, match=r"\((a|b)\)"):
        replay_forced_check(sd, z, tk2, forced, force, fed_stream(tk2, forced, force), lp2)
    with pytest.raises(AssertionError, match=r"\(c\)"):
        replay_forced_check(sd, z, tk2, forced, force, fed_stream(tk2, forced, force))


def test_forced_replay_rejects_swapped_rows(clean):
    """the results of two rows swapped from step 150 on (own tokens and log-probs; fed rebuilt from them, so the identity holds)"""
    sd, z, tk, lp, forced, force, fed, st = clean
    btk, blp = tk.clone(), lp.clone()
    btk[[3, 16], 150:] = tk[[16, 3], 150:]
    blp[[3, 16], 150:] = lp[[16, 3], 150:]
    assert not torch.equal(btk, tk)
    with pytest.raises(AssertionError, match=r"\(c\)"):
        replay_forced_check(sd, z, btk, forced, force, fed_stream(btk, forced, force))
    with pytest.raises(AssertionError, match=r"\((a|b)\)"):
        replay_forced_check(sd, z, btk, forced, force, fed_stream(btk, forced, force), blp)
    with pytest.raises(AssertionError, match=r"\(fed\)"):           # ... and with the fed stream left as it was
        replay_forced_check(sd, z, btk, forced, force, fed, blp)


def test_forced_cases_stay_under_the_near_tie_cap():
    """the GPU cases' inputs (helpers_forced.FORCED_CASES x the three masks; both batches of the graph paths), 8 sampled rows each, decoded
    by the fp32 oracle alone: every sample passes the checker, so the share of positions below delta is at most the cap"""
    inputs = {}
    for path, weights, Bi, steps in FORCED_CASES:
        if weights not in inputs:
            inputs[weights] = replay_inputs(weights)
        H, Z, sd = inputs[weights]
        for kind in FORCED_MASKS:
            for seed in ((Bi, Bi + 1) if path in FORCED_GRAPH_PATHS else (Bi,)):
                z = replay_z(Bi, Z, seed)
                rows = np.sort(np.random.RandomState(seed).choice(Bi, min(Bi, 8), replace=False))
                forced, force = forced_tokens(Bi, steps, seed)[rows], forced_mask(kind, steps, seed)
                lp, tk = oracle_forced_decode(sd, z[rows], steps, forced, force)
                st = replay_forced_check(sd, z[rows], tk, forced, force, fed_stream(tk, forced, force), lp)
                assert st["share_below_delta"] <= REPLAY_CAP
                print(forced_line("%s seed %d (oracle)" % (path, seed), kind, H, st))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. greedy_decode(..., forced, force) through FakeOps: scan-step path and both cells paths
# ------------------------------------------------------------------------------------------------------------------------------
def _fake_model(path):
    H, Z, sd = replay_inputs("h64")
    m = make_model(H, Z, sd, ops=FakeOps())
    m.eval()
    eng = m.engine()
    if path != "scan_steps":
        eng.cell_decode_rows = 1
    return m, sd, Z


FAKE_PATHS = [("scan_steps", True), ("cells", True), ("cells_fused_argmax", False)]


@pytest.mark.parametrize("path,want_logp", FAKE_PATHS)
@pytest.mark.parametrize("kind", FORCED_MASKS)
def test_forced_decode_on_the_per_token_paths(path, want_logp, kind):
    pkg = load_package()
    m, sd, Z = _fake_model(path)
    Bi, steps = 6, 60
    z = replay_z(Bi, Z, 11)
    forced, force = forced_tokens(Bi, steps + 3, 11), forced_mask(kind, steps, 11)       # wider than steps: only the first `steps` columns count
    lp, tk = pkg.greedy_decode(m, z, steps, want_logp=want_logp, forced=forced, force=force)
    assert (lp is None) == (not want_logp) and tk.dtype == torch.int32
    st = replay_forced_check(sd, z, tk, forced, force, pkg.fed_tokens(tk, forced, force), lp)
    print(forced_line(path + " (FakeOps)", kind, 64, st))
    if kind == "prefix":                                      # an int P = the first P steps
        P = int(force.sum())
        lp2, tk2 = pkg.greedy_decode(m, z, steps, want_logp=want_logp, forced=forced, force=P)
        assert torch.equal(tk, tk2) and (lp is None or torch.equal(lp, lp2))
        lp3, tk3 = pkg.continue_from(m, z, forced[:, :P], steps, want_logp=want_logp)
        assert torch.equal(tk3[:, :P].long(), forced[:, :P]) and torch.equal(tk3[:, P:], tk[:, P:]) and (lp is None or torch.equal(lp, lp3))
        assert torch.equal(tk3.long(), fed_stream(tk, forced, force))


@pytest.mark.parametrize("path,want_logp", FAKE_PATHS)
def test_forced_decode_ends(path, want_logp):
    """all-False = the plain call, bit for bit; all-True with forced = teacher = the oracle's teacher-forced log-probs"""
    pkg = load_package()
    m, sd, Z = _fake_model(path)
    Bi, steps = 6, 60
    z = replay_z(Bi, Z, 12)
    teacher = forced_tokens(Bi, steps, 12)
    lp0, tk0 = pkg.greedy_decode(m, z, steps, want_logp=want_logp)
    lp1, tk1 = pkg.greedy_decode(m, z, steps, want_logp=want_logp, forced=teacher, force=np.zeros(steps, bool))
    assert torch.equal(tk0, tk1) and (lp0 is None or torch.equal(lp0, lp1))
    lp2, tk2 = pkg.greedy_decode(m, z, steps, want_logp=want_logp, forced=teacher, force=[True] * steps)
    st = replay_forced_check(sd, z, tk2, teacher, np.ones(steps, bool), fed_stream(tk2, teacher, np.ones(steps, bool)), lp2)
    if want_logp:
        ref = orc.global_decoder({k: v.double() for k, v in sd.items()}, z.double(), steps, teacher=teacher)
        assert float((lp2.double() - ref).abs().max()) <= st["tol_lp"]


def test_forced_decode_argument_errors():
    pkg = load_package()
    m, sd, Z = _fake_model("scan_steps")
    z = replay_z(4, Z, 1)
    ok = forced_tokens(4, 20, 1)
    calls = []
    for name in ("gemm", "gru_seq_fwd", "gru_cell"):               # nothing may be launched before the arguments are accepted
        ops = m.engine().ops
        orig = getattr(ops, name)
        setattr(ops, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    bad = ok.clone()
    bad[2, 7] = 342
    neg = ok.clone()
    neg[0, 0] = -1
    for kw in (dict(forced=bad, force=10), dict(forced=neg, force=10),                     # token out of range
               dict(forced=ok, force=[True] * 19), dict(forced=ok, force=[True] * 21),     # short / long mask
               dict(forced=ok, force=21), dict(forced=ok, force=-1),
               dict(forced=ok[:3], force=10), dict(forced=ok[:, :19], force=10), dict(forced=ok[0], force=10),   # wrong shapes
               dict(forced=ok.float(), force=10), dict(forced=ok), dict(force=10)):
        with pytest.raises(ValueError):
            pkg.greedy_decode(m, z, 20, **kw)
    with pytest.raises(ValueError):
        pkg.greedy_decode(m, z, 0, forced=ok, force=0)             # no steps
    tk = forced_tokens(4, 20, 2)
    assert torch.equal(pkg.fed_tokens(tk, ok, 7), pkg.fed_tokens(tk, ok, [i < 7 for i in range(20)]))      # the int form of force
    assert torch.equal(pkg.fed_tokens(tk, ok, 7)[:, :7], ok[:, :7]) and torch.equal(pkg.fed_tokens(tk, ok, 7)[:, 7:], tk[:, 7:])
    assert torch.equal(pkg.fed_tokens(tk, ok, 0), tk)
    with pytest.raises(ValueError):
        pkg.fed_tokens(tk, ok, [True] * 19)
    with pytest.raises(ValueError):
        pkg.continue_from(m, z, ok[:, :5].repeat(1, 5), 20)        # prompt longer than the decode
    assert calls == []
    pkg.greedy_decode(m, z, 20, forced=ok, force=10)
    assert calls


def test_fader_sweep_prompt():
    """every (sample, value) row starts with the prompt and continues as continue_from does on that row's latent"""
    pkg = load_package()
    m, sd, Z = _fake_model("scan_steps")
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, 342, (2, 12), generator=g)
    chroma = torch.rand(2, 24, generator=g)
    eps = (torch.randn(2, Z, generator=g), torch.randn(2, Z, generator=g))
    prompt = torch.tensor([5, 77, 200, 9])
    tok, z0 = pkg.fader_sweep(m, x, chroma, [-1.0, 0.5, 2.0], steps=16, eps=eps, prompt=prompt)
    plain, z0p = pkg.fader_sweep(m, x, chroma, [-1.0, 0.5, 2.0], steps=16, eps=eps)
    assert tuple(tok.shape) == (2, 3, 16) and torch.equal(z0, z0p)
    assert torch.equal(tok[:, :, :4].long(), prompt.view(1, 1, 4).expand(2, 3, 4))
    assert not torch.equal(tok[:, :, 4:], plain[:, :, 4:])


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the host twin under ASAN, 4. the ABI without a GPU
# ------------------------------------------------------------------------------------------------------------------------------
def test_forced_host_twin_under_asan():
    lib = os.path.join(ROOT, "music-fader-nets_amd", "libfadernets_host.so")
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    assert os.path.exists(lib), "libfadernets_host.so missing although the sanitizer toolchain is there: the host twins did not build"
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_forced_driver.py")], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0 and "HOST FORCED DECODE OK" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
    assert "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    print(p.stdout)


def test_forced_entry_point_argument_errors_without_gpu():
    load_package()
    from music_fader_nets_amd import _lib
    lib = _lib.load()
    assert lib.fn_version() == 6
    d, f = _lib.FnDecode(), _lib.FnDecodeForce()
    assert lib.fn_decode_forced(None, None, None) == -1
    assert lib.fn_decode_forced(None, C.byref(f), None) == -1
    assert lib.fn_decode_forced(C.byref(d), None, None) == -1
    assert lib.fn_decode_forced(C.byref(d), C.byref(f), None) == -1          # f->force / f->forced NULL
    hdr = open(os.path.join(ROOT, "include", "fadernets.h")).read()
    assert "gmm_model.py:139-148" in hdr and "fn_decode_forced_host" in open(os.path.join(ROOT, "include", "fadernets_host.h")).read()
