"""Seeded temperature / top-k / top-p sampling decode (decode.sample_decode, fn_vocab_sample), CPU side: Philox known answers, the checker of
drawn tokens against planted faults, the near-boundary cap of the inputs the GPU tests use, the per-token paths through a FakeOps stand-in,
the host twin in a stand-alone sanitizer build, the ABI's argument answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import REPLAY_CAP, make_model, replay_inputs, replay_z
from helpers_forced import forced_tokens
from helpers_sampling import (PARAMS_DTYPE, SETTINGS, SamplingFakeOps, oracle_sample_decode, philox4x32_10, reference_sample, sample_check,
                              sample_check_decode, sample_line, sample_rows, sample_uniforms)
from mfn_import import ROOT, load_package

V = 342


def _params(s, **kw):
    return dict(T=s[0], k=s[1], p=s[2], **kw)


def _synthetic(N, seed, std=8.0, v=V):
    """log-prob rows of N(0, std^2) logits, as the fp32 log_softmax leaves them"""
    x = torch.randn(N, v, generator=torch.Generator().manual_seed(seed)) * std
    return torch.log_softmax(x, dim=-1).numpy()


# ------------------------------------------------------------------------------------------------------------------------------
# 1. Philox4x32-10
# ------------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for ctr, key, out in (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                          ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                          ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")):
        got = philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert " ".join("%08x" % int(w) for w in got) == out
    u = sample_uniforms([0, 3], [0, 5], seed=(7 << 32) | 9, offset=(1 << 40) | 2)
    assert u.dtype == np.float32 and u.shape == (2, 2) and (u >= 0).all() and (u < 1).all()
    w = philox4x32_10(np.array([3, 5, 2, 1 << 8], dtype=np.uint32), np.array([9, 7], dtype=np.uint32))[0]
    assert u[1, 1] == np.float32(int(w) >> 8) * np.float32(2.0 ** -24)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the checker
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean():
    """24 rows x 40 steps of synthetic log-probs, drawn by the fp32 restatement with (0.8, 40, 0.95), seed 11, offset 5"""
    s = SETTINGS[4]
    par = _params(s, seed=11, offset=5)
    B, steps = 24, 40
    lp = _synthetic(B * steps, 1).reshape(B, steps, V)
    u = sample_uniforms(np.arange(B), np.arange(steps), 11, 5)
    r = sample_rows(lp.reshape(-1, V), u.reshape(-1), *s, dtype=np.float32)
    tok = r["tok"].reshape(B, steps)
    st = sample_check_decode(lp, tok, np.arange(B), par)
    return lp, tok, u, par, st, r


def test_sample_check_accepts_the_reference(clean):
    lp, tok, u, par, st, r = clean
    assert st["positions"] == 24 * 40 and 0 < st["e_cdf"] < 1e-5 and st["delta"] == min(1e-4, 16 * st["e_cdf"]) and st["share_near"] <= REPLAY_CAP
    assert int((r["m"] < 40).sum()) > 0 and int(r["m"].max()) <= 40                       # top-p cuts inside the top-k prefix
    assert reference_sample(lp[3, 7], u[3, 7], *SETTINGS[4], dtype=np.float32) == tok[3, 7]
    assert len(np.unique(tok)) > 20


def test_sample_check_rejects_planted_faults(clean):
    lp, tok, u, par, st, r = clean
    B, steps = tok.shape
    far = ~st["near"]
    order, m = r["order"].reshape(B, steps, V), r["m"].reshape(B, steps)
    rank = np.argsort(order, axis=-1)
    # a token moved to its neighbour in the sorted order, at a position that is not near
    b, i = (int(x) for x in np.argwhere(far & (m >= 3))[17])
    j = int(rank[b, i, tok[b, i]])
    bad = tok.copy()
    bad[b, i] = order[b, i, j + 1 if j + 1 < m[b, i] else j - 1]
    with pytest.raises(AssertionError, match=r"\(tok\)"):
        sample_check_decode(lp, bad, np.arange(B), par)
    # a token outside the top-k prefix
    bad = tok.copy()
    bad[b, i] = order[b, i, 45]
    with pytest.raises(AssertionError, match=r"\(tok\)"):
        sample_check_decode(lp, bad, np.arange(B), par)
    # step i's uniforms used at step i + 1
    us = np.concatenate([u[:, :1], u[:, :-1]], axis=1)
    bad = sample_rows(lp.reshape(-1, V), us.reshape(-1), *SETTINGS[4], dtype=np.float32)["tok"].reshape(B, steps)
    assert (bad != tok).mean() > 0.1
    with pytest.raises(AssertionError, match=r"\(tok\)"):
        sample_check_decode(lp, bad, np.arange(B), par)
    # two rows' tokens swapped
    bad = tok.copy()
    bad[[3, 16]] = tok[[16, 3]]
    with pytest.raises(AssertionError, match=r"\(tok\)"):
        sample_check_decode(lp, bad, np.arange(B), par)
    # ... and the same rows under their true numbers pass where they sit in a subset
    sample_check_decode(lp[[3, 16]], tok[[3, 16]], np.array([3, 16]), par)
    # an offset that is ignored
    u0 = sample_uniforms(np.arange(B), np.arange(steps), 11, 0)
    bad = sample_rows(lp.reshape(-1, V), u0.reshape(-1), *SETTINGS[4], dtype=np.float32)["tok"].reshape(B, steps)
    with pytest.raises(AssertionError, match=r"\(tok\)"):
        sample_check_decode(lp, bad, np.arange(B), par)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the inputs stay under the near-boundary cap (fp32 restatement against fp64)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SETTINGS, ids=["T%g-k%d-p%g" % s for s in SETTINGS])
def test_synthetic_rows_stay_under_the_near_cap(s):
    lp = _synthetic(1500, 2)
    u = sample_uniforms(np.arange(1500), [0], 3, 0)[:, 0]
    tok = sample_rows(lp, u, *s, dtype=np.float32)["tok"]
    st = sample_check(lp, tok, u, _params(s))
    print(sample_line("synthetic N(0, 64)", _params(s), st))
    assert st["share_near"] <= REPLAY_CAP


@pytest.fixture(scope="module")
def weights():
    return {w: replay_inputs(w) for w in ("h64", "h512")}


@pytest.mark.parametrize("w", ["h64", "h512"])
def test_model_rows_stay_under_the_near_cap(weights, w):
    H, Z, sd = weights[w]
    Bi, steps = 8, 48
    z = replay_z(Bi, Z, 21)
    for n, s in enumerate(SETTINGS):
        par = _params(s, seed=100 + n, offset=n)
        lp, tok = oracle_sample_decode(sd, z, steps, *s, seed=par["seed"], offset=par["offset"])
        st = sample_check_decode(lp, tok, np.arange(Bi), par)
        print(sample_line("oracle %s" % w, par, st))
        assert st["share_near"] <= REPLAY_CAP


# ------------------------------------------------------------------------------------------------------------------------------
# 4. sample_decode through the stand-in, both per-token branches
# ------------------------------------------------------------------------------------------------------------------------------
def _fake_model(path):
    H, Z, sd = replay_inputs("h64")
    m = make_model(H, Z, sd, ops=SamplingFakeOps())
    m.eval()
    if path == "cells":
        m.engine().cell_decode_rows = 1
    return m, sd, Z


def _upto_first_near(tok, ref, near):
    """tokens equal in every row up to its first near position (a draw that may fall either way sends the rest of the row elsewhere)"""
    for b in range(tok.shape[0]):
        hit = np.nonzero(near[b])[0]
        end = int(hit[0]) if len(hit) else tok.shape[1]
        assert np.array_equal(np.asarray(tok[b, :end]), np.asarray(ref[b, :end])), b


@pytest.mark.parametrize("path", ["scan_steps", "cells"])
def test_sample_decode_on_the_per_token_paths(path):
    pkg = load_package()
    m, sd, Z = _fake_model(path)
    Bi, steps = 6, 40
    z = replay_z(Bi, Z, 13)
    for n, s in enumerate(SETTINGS[:1] + SETTINGS[4:]):
        par = _params(s, seed=(5 << 32) + n, offset=(1 << 33) + n)
        kw = dict(temperature=s[0], top_k=s[1], top_p=s[2], seed=par["seed"], offset=par["offset"])
        lp, tk = pkg.sample_decode(m, z, steps, **kw)
        assert tk.dtype == torch.int32 and tuple(tk.shape) == (Bi, steps) and tuple(lp.shape) == (Bi, steps, V)
        st = sample_check_decode(lp, tk, np.arange(Bi), par)
        lpo, tko = oracle_sample_decode(sd, z, steps, *s, seed=par["seed"], offset=par["offset"])
        sto = sample_check_decode(lpo, tko, np.arange(Bi), par)
        _upto_first_near(tk.numpy(), tko.numpy(), st["near"] | sto["near"])
        # the same seed again, tokens only; another seed, another offset
        lp2, tk2 = pkg.sample_decode(m, z, steps, want_logp=False, **kw)
        assert lp2 is None and torch.equal(tk2, tk)
        assert not torch.equal(pkg.sample_decode(m, z, steps, **dict(kw, seed=par["seed"] + 1))[1], tk)
        assert not torch.equal(pkg.sample_decode(m, z, steps, **dict(kw, offset=par["offset"] + 1))[1], tk)
    # top_k = 1 is the greedy decode
    lpg, tkg = pkg.greedy_decode(m, z, steps)
    lp1, tk1 = pkg.sample_decode(m, z, steps, temperature=0.7, top_k=1, seed=3)
    assert torch.equal(tk1, tkg) and torch.equal(lp1, lpg)
    # a prompt: its tokens are the stream's first columns, the draws after it follow them
    P = steps // 3
    prompt = forced_tokens(Bi, P, 13)
    par = _params(SETTINGS[4], seed=8, offset=0)
    lp, tk = pkg.sample_decode(m, z, steps, temperature=0.8, top_k=40, top_p=0.95, seed=8, prompt=prompt)
    assert torch.equal(tk[:, :P].long(), prompt)
    st = sample_check_decode(lp, tk, np.arange(Bi), par, P=P)
    lpo, tko = oracle_sample_decode(sd, z, steps, *SETTINGS[4], seed=8, prompt=prompt)
    sto = sample_check_decode(lpo, tko, np.arange(Bi), par, P=P)
    _upto_first_near(tk.numpy(), tko.numpy(), st["near"] | sto["near"])
    assert float((lp - lpo).abs().max()) < 1e-4 or (st["near"] | sto["near"]).any()
    assert not torch.equal(tk[:, P:], pkg.sample_decode(m, z, steps, temperature=0.8, top_k=40, top_p=0.95, seed=8)[1][:, P:])


def test_sample_decode_leaves_the_greedy_launches_alone():
    """the greedy and forced branches issue what they issued: no sampling op in their call log, and the sampling decode never the argmax head"""
    pkg = load_package()
    m, sd, Z = _fake_model("scan_steps")
    ops = m.engine().ops
    z = replay_z(4, Z, 2)
    pkg.greedy_decode(m, z, 10)
    pkg.continue_from(m, z, forced_tokens(4, 3, 2), 10)
    assert "vocab_sample" not in ops.calls
    seen = []
    ops.vocab_argmax = lambda *a, **k: seen.append("vocab_argmax")
    ops.out_argmax = lambda *a, **k: seen.append("out_argmax")
    pkg.sample_decode(m, z, 10, want_logp=False)
    assert ops.calls.count("vocab_sample") == 10 and not seen


def test_fader_sweep_sample():
    pkg = load_package()
    m, sd, Z = _fake_model("scan_steps")
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, V, (2, 12), generator=g)
    chroma = torch.rand(2, 24, generator=g)
    eps = (torch.randn(2, Z, generator=g), torch.randn(2, Z, generator=g))
    prompt = torch.tensor([5, 77, 200, 9])
    plain, z0 = pkg.fader_sweep(m, x, chroma, [-1.0, 0.5, 2.0], steps=16, eps=eps)
    a, z0a = pkg.fader_sweep(m, x, chroma, [-1.0, 0.5, 2.0], steps=16, eps=eps, sample=dict(temperature=1.2, seed=4))
    b, _ = pkg.fader_sweep(m, x, chroma, [-1.0, 0.5, 2.0], steps=16, eps=eps, sample=dict(temperature=1.2, seed=4))
    c, _ = pkg.fader_sweep(m, x, chroma, [-1.0, 0.5, 2.0], steps=16, eps=eps, sample=dict(temperature=1.2, seed=5), prompt=prompt)
    assert tuple(a.shape) == (2, 3, 16) and torch.equal(z0, z0a) and torch.equal(a, b) and not torch.equal(a, plain)
    assert torch.equal(c[:, :, :4].long(), prompt.view(1, 1, 4).expand(2, 3, 4)) and not torch.equal(c[:, :, 4:], a[:, :, 4:])
    k1, _ = pkg.fader_sweep(m, x, chroma, [-1.0, 0.5, 2.0], steps=16, eps=eps, sample=dict(top_k=1))
    assert torch.equal(k1, plain)
    for bad in (dict(want_logp=True), dict(prompt=prompt), dict(temprature=1.0), dict(temperature=0.0)):       # ValueError, as sample_decode's own
        with pytest.raises(ValueError):
            pkg.fader_sweep(m, x, chroma, [-1.0, 0.5, 2.0], steps=16, eps=eps, sample=bad)


def test_sample_decode_argument_errors():
    pkg = load_package()
    m, sd, Z = _fake_model("scan_steps")
    z = replay_z(4, Z, 1)
    ops = m.engine().ops
    calls = []
    for name in ("gemm", "gru_seq_fwd", "gru_cell", "vocab_sample"):          # nothing may be launched before the arguments are accepted
        orig = getattr(ops, name)
        setattr(ops, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    ok = forced_tokens(4, 5, 1)
    bad = ok.clone()
    bad[1, 2] = V
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(temperature="1"),
               dict(top_k=-1), dict(top_k=2.5), dict(top_k=1 << 31), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(top_p=-0.1),
               dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5), dict(offset=-1), dict(offset=1 << 64),
               dict(prompt=bad), dict(prompt=-ok), dict(prompt=ok[:3]), dict(prompt=ok[0]), dict(prompt=ok.float()), dict(prompt=ok.repeat(1, 5))):
        with pytest.raises(ValueError):
            pkg.sample_decode(m, z, 20, **kw)
    with pytest.raises(ValueError):
        pkg.sample_decode(m, z, 0)
    assert calls == [] and ops.calls == []
    pkg.sample_decode(m, z, 20, temperature=1e-3, top_k=500, top_p=1.0, seed=(1 << 64) - 1, offset=(1 << 64) - 1, prompt=ok)
    assert "vocab_sample" in calls and "gemm" in calls


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the host twin in a stand-alone sanitizer build, 6. the ABI without a GPU
# ------------------------------------------------------------------------------------------------------------------------------

def _run_twin(exe, tmp_path, x, s, step, seed, offset, ld=None):
    B, v = x.shape
    ld = ld or v
    buf = np.zeros((B, ld), dtype=np.float32)
    buf[:, :v] = x
    raw = np.zeros(1, dtype=PARAMS_DTYPE)
    raw["seed"], raw["offset"], raw["inv_t"], raw["top_p"], raw["top_k"] = seed, offset, np.float32(1.0) / np.float32(s[0]), s[2], s[1]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([B, v, ld, step], dtype=np.int32).tobytes() + raw.tobytes() + buf.tobytes())
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    out = open(fout, "rb").read()
    assert np.frombuffer(out[:4], dtype=np.int32)[0] == 0 and len(out) == 4 + 12 * B + 4 * B * v
    tok, own = np.frombuffer(out[4:4 + 4 * B], dtype=np.int32), np.frombuffer(out[4 + 4 * B:4 + 8 * B], dtype=np.int32)
    u = np.frombuffer(out[4 + 8 * B:4 + 12 * B], dtype=np.float32)
    lp = np.frombuffer(out[4 + 12 * B:], dtype=np.float32).reshape(B, v)
    return tok, own, u, lp


def test_host_twin_stand_alone_under_sanitizers(tmp_path):
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    src = os.path.join(ROOT, "music-fader-nets_amd", "csrc", "host", "sample_check.cpp")
    exe = str(tmp_path / "sample_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror", src, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    gen = torch.Generator().manual_seed(9)
    cases = [(9, V, s, V + 2) for s in SETTINGS] + [(1, 1024, SETTINGS[4], None), (1, 1, SETTINGS[4], None), (1, 1024, SETTINGS[0], None)]
    for n, (B, v, s, ld) in enumerate(cases):
        x = (torch.randn(B, v, generator=gen) * 8).numpy()
        seed, offset, step = (3 << 32) + n, (1 << 35) + n, 5 * (n % 2)
        tok, own, u, lp = _run_twin(exe, tmp_path, x, s, step, seed, offset, ld)
        assert np.array_equal(u.view(np.uint32), sample_uniforms(np.arange(B), [step], seed, offset)[:, 0].view(np.uint32))
        assert np.array_equal(own, x.argmax(1)) and np.abs(lp - torch.log_softmax(torch.from_numpy(x), -1).numpy()).max() < 1e-4
        st = sample_check(lp, tok, u, _params(s))
        print(sample_line("host twin B %d V %d" % (B, v), _params(s), st))


def test_vocab_sample_argument_errors_without_gpu():
    load_package()
    from music_fader_nets_amd import _lib
    lib = _lib.load()
    assert lib.fn_version() == 6 and C.sizeof(_lib.FnSampleParams) == 32
    x = (C.c_float * 2048)()
    par = _lib.FnSampleParams()
    tok = (C.c_int32 * 4)()
    px, pp, pt = (C.cast(o, C.c_void_p) for o in (x, C.pointer(par), tok))
    assert lib.fn_vocab_sample(None, 1, V, V, pp, 0, None, 0, None, 0, pt, 1, None, None) == -1
    assert lib.fn_vocab_sample(px, 1, V, V, None, 0, None, 0, None, 0, pt, 1, None, None) == -1
    assert lib.fn_vocab_sample(px, 1, V, V, pp, 0, None, 0, None, 0, None, 1, None, None) == -1
    assert lib.fn_vocab_sample(px, 1, 0, 8, pp, 0, None, 0, None, 0, pt, 1, None, None) == -2
    assert lib.fn_vocab_sample(px, 1, 1025, 1025, pp, 0, None, 0, None, 0, pt, 1, None, None) == -2
    assert lib.fn_vocab_sample(px, 0, V, V, pp, 0, None, 0, None, 0, pt, 1, None, None) == -2
    assert lib.fn_vocab_sample(px, 1, V, V - 1, pp, 0, None, 0, None, 0, pt, 1, None, None) == -2
    assert _lib.FN_SAMPLE_MAX_V == 1024
    hdr = open(os.path.join(ROOT, "include", "fadernets.h")).read()
    assert "NO reference counterpart" in hdr and "fn_vocab_sample_host" in open(os.path.join(ROOT, "include", "fadernets_host.h")).read()
