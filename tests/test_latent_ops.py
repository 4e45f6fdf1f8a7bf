"""Generation from the mixture prior and morphing (latent.py, fn_latent_draw / fn_latent_mix), CPU side: the Philox known answer, the statistics of the
drawn normals, the host twins in a stand-alone sanitizer build against the float64 restatement on the case lists, the exact cases, the entry points'
answers to bad arguments, and the Python layer on stand-in ops."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers_latent_ops as hl
from helpers import make_model
from mfn_import import ROOT, load_package


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the restatement
# ------------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answer():
    got = hl.philox4x32_10(np.zeros(4, np.uint32), np.zeros(2, np.uint32))
    assert [int(v) for v in got] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(v) for v in hl._words(1, [0], 0, 0)[0, 0]] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]          # the draw's counter layout at row 0, quad 0
    # the counter words are (row, (stream << 16) | quad, offset_lo, offset_hi), the key is the seed
    w = hl._words(4, [(3 << 16) | 5], (9 << 32) | 7, (2 << 32) | 1)[3, 0]
    assert np.array_equal(w, hl.philox4x32_10(np.array([3, (3 << 16) | 5, 1, 2], np.uint32), np.array([7, 9], np.uint32)))


def test_draw_statistics_of_the_restatement():
    rows, Z = 4096, 128
    for seed in (2024, 7):
        n0, n1 = hl.draw_normals(rows, Z, 0, seed)[0], hl.draw_normals(rows, Z, 1, seed)[0]
        figures, corr = hl.stats_ok(n0, n1)
        print("seed %d: (mean, var, m4) %s corr %.2e" % (seed, figures, corr))
        assert np.abs(n0).max() <= np.sqrt(48 * np.log(2)) and not np.array_equal(n0, n1)
        for K in (2, 3, 8):
            for stream in (0, 1):
                print("seed %d K %d stream %d counts %s" % (seed, K, stream, hl.counts_ok(hl.draw_components(rows, K, stream, seed), K).tolist()))
    # a row's numbers do not depend on the number of rows, and a last quad drops its rest
    assert np.array_equal(hl.draw_normals(3, 5, 1, 7)[0], hl.draw_normals(rows, Z, 1, 7)[0][:3, :5])


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the host twins in a stand-alone sanitizer build
# ------------------------------------------------------------------------------------------------------------------------------
def _run(exe, fin, fout, blob):
    with open(fin, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    return open(fout, "rb").read()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    tmp = tmp_path_factory.mktemp("latent_ops")
    src = os.path.join(ROOT, "music-fader-nets_amd", "csrc", "host", "latent_ops_check.cpp")
    exe = str(tmp / "latent_ops_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror", src, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return lambda blob: _run(exe, str(tmp / "in.bin"), str(tmp / "out.bin"), blob)


def _twin_mix(twin):
    def run(a, b, t, segs, per_pair=False, ab_ld=None, out_ld=None):
        c = dict(tag="exact", a=a, b=b, t=np.asarray(t, np.float32), segs=segs, per_pair=per_pair, ab_ld=ab_ld or a.shape[1], out_ld=out_ld or a.shape[1])
        return hl.parse_mix(c, twin(hl.mix_blob(c)))
    return run


def test_host_twin_draw_against_the_restatement(twin):
    worst = [0.0, 0.0]
    for c in hl.draw_cases():
        z, eps, comp = hl.parse_draw(c, twin(hl.draw_blob(c)))
        worst = [max(x, y) for x, y in zip(worst, hl.check_draw_case(c, z, eps, comp))]
    print("twin draw: worst error / bound, eps %.3f z %.3f" % tuple(worst))
    # without the optional outputs the z buffer is the same
    c = hl.draw_cases()[4]
    full = hl.parse_draw(c, twin(hl.draw_blob(c)))[0]
    raw = twin(hl.draw_blob(c, flags=1))
    assert np.array_equal(np.frombuffer(raw[4:], np.float32), full) and np.frombuffer(raw[:4], np.int32)[0] == 0


def test_host_twin_draw_statistics(twin):
    mu, lv = np.zeros((2, 128), np.float32), np.zeros((2, 128), np.float32)
    for seed in (2024, 7):
        c = dict(tag="stats", rows=4096, Z=128, z_ld=256, col_step=128, tau=1.0, seed=seed, offset=0,
                 jobs=[dict(mu_lk=mu, lv_lk=lv, comp=None, stream_id=s) for s in (0, 1)])
        z, eps, comp = hl.parse_draw(c, twin(hl.draw_blob(c)))
        hl.stats_ok(eps[0], eps[1])
        assert np.array_equal(z.reshape(4096, 256)[:, :128], eps[0]) and np.array_equal(z.reshape(4096, 256)[:, 128:], eps[1])          # mu 0, sigma 1, tau 1
        for s in (0, 1):
            hl.counts_ok(comp[s], 2)


def test_host_twin_mix_against_float64(twin):
    worst = 0.0
    for c in hl.mix_cases():
        out, omega = hl.parse_mix(c, twin(hl.mix_blob(c)))
        worst = max(worst, hl.check_mix(c["a"], c["b"], c["t"], c["segs"], out, omega, c["per_pair"], c["tag"]))
    print("twin mix: max |out - out64| / (|a| + |b|) = %.3e" % worst)
    assert worst <= hl.MIX_TOL


def test_host_twin_exact_cases(twin):
    hl.exact_mix_checks(_twin_mix(twin))


def test_host_twin_answers_to_bad_sizes(twin):
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    rc = lambda blob: np.frombuffer(twin(blob), np.int32).tolist()
    par = hl.params_bytes().tobytes()
    job = lambda K, sid, Z: i32(K, sid) + np.zeros(2 * max(K, 0) * max(Z, 0), np.float32).tobytes()
    #          n_jobs rows Z z_ld   K  stream
    for hd, want in (((0, 2, 4, 4, 2, 0), -5), ((5, 2, 4, 4, 2, 0), -5), ((1, 0, 4, 4, 2, 0), -2), ((1, 2, 0, 4, 2, 0), -2), ((1, 2, 4, 3, 2, 0), -2),
                     ((1, 2, 4, 4, 0, 0), -2), ((1, 2, 4, 4, 2, -1), -2), ((1, 2, 4, 4, 2, 65535), -2), ((1, 1, 4097, 4097, 1, 0), -6),
                     ((1, 1, 4, 4, 1025, 0), -6)):
        n_jobs, rows, Z, z_ld, K, sid = hd
        assert rc(i32(0, n_jobs, rows, Z, z_ld, 0, 6, 0) + par + job(K, sid, Z) * min(max(n_jobs, 0), 8)) == [want], hd
    #          pairs D ab_ld P n_segs out_ld, segs
    for hd, segs, want in (((1, 4, 4, 1, 0, 4), [], -5), ((1, 4, 4, 1, 5, 4), [(0, 1, 0)] * 5, -5), ((0, 4, 4, 1, 1, 4), [(0, 4, 0)], -2),
                           ((1, 0, 4, 1, 1, 4), [(0, 4, 0)], -2), ((1, 4, 4, 0, 1, 4), [(0, 4, 0)], -2), ((1, 4, 3, 1, 1, 4), [(0, 4, 0)], -2),
                           ((1, 4, 4, 1, 1, 3), [(0, 4, 0)], -2), ((1, 4, 4, 1, 1, 4), [(1, 4, 0)], -2), ((1, 4, 4, 1, 1, 4), [(-1, 2, 0)], -2),
                           ((1, 4, 4, 1, 1, 4), [(0, 0, 0)], -2), ((1, 4, 4, 1, 1, 4), [(0, 4, 3)], -2), ((1, 4, 4, 1, 1, 4), [(0, 4, -1)], -2),
                           ((1, 4, 4, 1, 2, 4), [(0, 3, 0), (2, 2, 1)], -2), ((1, 4, 4, 1, 2, 4), [(2, 2, 0), (0, 3, 1)], -2)):
        pairs, D, ab_ld, P, n_segs, out_ld = hd
        n_ab = (pairs - 1) * ab_ld + D if pairs > 0 else 0
        blob = i32(1, pairs, D, ab_ld, P, 0, n_segs, out_ld) + b"".join(i32(*s, 0) for s in segs) + np.zeros(2 * max(n_ab, 0) + max(P, 0), np.float32).tobytes()
        assert rc(blob) == [want], (hd, segs)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the ABI without a GPU
# ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_argument_errors_without_gpu():
    load_package()
    from music_fader_nets_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "fadernets.h")).read()
    for name, text in (("FN_DRAW_MAX_JOBS", "4"), ("FN_DRAW_MAX_Z", "4096"), ("FN_DRAW_MAX_K", "1024"), ("FN_MIX_LERP", "0"), ("FN_MIX_SLERP", "1"),
                       ("FN_MIX_STEP", "2"), ("FN_MIX_MAX_SEGS", "4"), ("FN_MIX_MIN_SIN", "1e-4f")):
        assert re.search(r"^#define %s %s$" % (name, re.escape(text)), hdr, re.M) and float(text.rstrip("f")) == getattr(_lib, name), name
    assert (C.sizeof(_lib.FnDrawParams), C.sizeof(_lib.FnDrawJob), C.sizeof(_lib.FnMixSeg)) == (32, 56, 16) and lib.fn_version() == 6
    assert {"fn_latent_draw", "fn_latent_mix"} <= set(_lib.SIGNATURES)
    twins = open(os.path.join(ROOT, "include", "fadernets_host.h")).read()
    assert "fn_latent_draw_host" in twins and "fn_latent_mix_host" in twins
    buf = (C.c_int32 * 4096)()
    at = (C.addressof(buf) + 15) // 16 * 16
    odd = at + 2

    def draw(n_jobs=2, rows=3, Z=8, z_ld=40, params=at, jobs=True, **kw):
        arr = (_lib.FnDrawJob * 5)()
        for j in arr:
            j.mu_lk, j.lv_lk, j.comp, j.z, j.eps_out, j.comp_out, j.K, j.stream_id = at, at, None, at, None, None, 2, 1
        for k, v in kw.items():
            setattr(arr[1], k, v)                                             # the second job carries the fault
        return lib.fn_latent_draw(arr if jobs else None, n_jobs, rows, Z, z_ld, params, None)

    assert draw(jobs=False) == -1 and draw(params=None) == -1
    for k in ("mu_lk", "lv_lk", "z"):
        assert draw(**{k: None}) == -1, k
    assert draw(n_jobs=0) == -5 and draw(n_jobs=5) == -5 and draw(n_jobs=-1) == -5
    for kw in (dict(rows=0), dict(rows=-1), dict(Z=0), dict(z_ld=7), dict(K=0), dict(K=-3), dict(stream_id=-1), dict(stream_id=65535)):
        assert draw(**kw) == -2, kw
    for kw in (dict(Z=4097, z_ld=4097), dict(K=1025), dict(rows=(1 << 31) - 1, Z=8)):
        assert draw(**kw) == -6, kw
    for k in ("mu_lk", "lv_lk", "comp", "z", "eps_out", "comp_out"):
        assert draw(**{k: odd}) == -3, k
    assert draw(params=odd) == -3
    # the order: null pointers first (in every job the count admits), then the count, the sizes, the limits, the alignment
    assert draw(n_jobs=5, z=None) == -1 and draw(n_jobs=0, params=None) == -1 and draw(rows=0, mu_lk=None) == -1
    assert draw(n_jobs=5, rows=0) == -5 and draw(rows=0, Z=4097, z_ld=4097) == -2 and draw(K=1025, z=odd) == -6 and draw(K=0, z=odd) == -2

    def mix(a=at, b=at, ab_ld=16, pairs=2, D=12, t=at, P=3, per_pair=0, segs=((0, 4, 1), (4, 4, 0), (8, 4, 2)), n_segs=None, out=at, out_ld=16, omega=at, no_segs=False):
        arr = (_lib.FnMixSeg * 8)()
        for s, v in zip(arr, segs):
            s.off, s.len, s.mode = v
        return lib.fn_latent_mix(a, b, ab_ld, pairs, D, t, P, per_pair, None if no_segs else arr, len(segs) if n_segs is None else n_segs, out, out_ld, omega, None)

    for k in ("a", "b", "t", "out"):
        assert mix(**{k: None}) == -1, k
    assert mix(no_segs=True) == -1
    assert mix(n_segs=0) == -5 and mix(n_segs=5) == -5
    for kw in (dict(pairs=0), dict(D=0), dict(P=0), dict(ab_ld=11), dict(out_ld=11), dict(segs=((0, 13, 0),)), dict(segs=((-1, 4, 0),)), dict(segs=((12, 1, 0),)),
               dict(segs=((0, 0, 0),)), dict(segs=((0, 4, 3),)), dict(segs=((0, 4, -1),)), dict(segs=((0, 4, 0), (3, 4, 0))), dict(segs=((4, 4, 0), (0, 12, 0))),
               dict(segs=((0, 4, 0), (0, 4, 0)))):
        assert mix(**kw) == -2, kw
    assert mix(pairs=1 << 16, P=1 << 15) == -6
    for k in ("a", "b", "t", "out", "omega"):
        assert mix(**{k: odd}) == -3, k
    assert mix(a=None, n_segs=0) == -1 and mix(n_segs=0, pairs=0) == -5 and mix(pairs=0, a=odd) == -2 and mix(pairs=1 << 16, P=1 << 15, a=odd) == -6


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the Python layer on stand-ins
# ------------------------------------------------------------------------------------------------------------------------------
def test_python_value_errors_come_before_any_launch():
    pkg = load_package()
    ops = hl.latent_fake_ops()
    m = make_model(64, 8, ops=ops)
    made = []
    m.encode = lambda *a, **k: made.append("encode")
    ok = dict(rows=4, key=3)
    for kw in (dict(rows=0), dict(rows=2.0), dict(rows=True), dict(rows=None), dict(rhythm=2), dict(rhythm=-1), dict(rhythm=1.0), dict(rhythm=[0, 1, 0]),
               dict(rhythm=np.zeros(4)), dict(rhythm=[0, 1, 2, 0]), dict(note="x"), dict(note=[True] * 4), dict(note=torch.tensor([0, 0, 0, -1])),
               dict(chroma=np.zeros(24)), dict(key=None), dict(key=24), dict(key=-1), dict(key=1.5), dict(key=None, chroma=np.zeros(23)),
               dict(key=None, chroma=np.zeros((5, 24))), dict(key=None, chroma="c"), dict(temperature=-1.0), dict(temperature=float("nan")),
               dict(temperature=float("inf")), dict(temperature="1"), dict(seed=-1), dict(seed=1 << 64), dict(seed=1.0), dict(offset=1.5), dict(offset=-1)):
        for fn in (pkg.prior_latents, pkg.generate):
            with pytest.raises(ValueError):
                fn(m, **dict(ok, **kw))
    for kw in (dict(steps=0), dict(steps=2.5), dict(beam=dict(width=2), sample=dict(seed=1)), dict(beam=dict(depth=2)), dict(beam=dict(width=17)),
               dict(beam=dict(width=2), prompt=[2, 3]), dict(sample=dict(temp=1.0)), dict(constraints="x")):
        with pytest.raises(ValueError):
            pkg.generate(m, **dict(ok, **kw))
    D = 2 * 8 + 24
    za, zb = torch.zeros(3, D), torch.ones(3, D)
    for kw in (dict(za=torch.zeros(3, D - 1)), dict(za=torch.zeros(3, D, dtype=torch.int32)), dict(zb=torch.zeros(2, D)), dict(za=za.numpy()), dict(za=torch.zeros(D)),
               dict(t=[]), dict(t=[float("nan")]), dict(t=[0.0, float("inf")]), dict(t=[[0.0, 1.0]]), dict(t="ab"), dict(t=None), dict(mode="cubic"), dict(mode=1),
               dict(per_pair=1), dict(per_pair=True, t=[0.0, 1.0]), dict(per_pair=True, t=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            pkg.mix_latents(m, **dict(dict(za=za, zb=zb, t=[0.0, 0.5]), **kw))
    xa, ca = torch.zeros(2, 20, dtype=torch.int64), torch.zeros(2, 24)
    e = torch.zeros(4, 8)
    for kw in (dict(points=0), dict(points=1.5), dict(points=True), dict(xb=torch.zeros(2, 21, dtype=torch.int64)), dict(xb=torch.zeros(3, 20, dtype=torch.int64)),
               dict(xa=xa.numpy()), dict(ca=torch.zeros(2, 23)), dict(cb=torch.zeros(3, 24)), dict(eps=(e,)), dict(eps=(e, e[:2])), dict(eps=(e, torch.zeros(4, 9))),
               dict(eps=e), dict(t=[float("nan")]), dict(t=[]), dict(mode="step"), dict(steps=0), dict(beam=dict(width=2), sample=dict(seed=1)),
               dict(sample=dict(tau=1.0)), dict(constraints=3)):
        with pytest.raises(ValueError):
            pkg.morph(m, **dict(dict(xa=xa, ca=ca, xb=xa, cb=ca), **kw))
    for z in (torch.zeros(3, D + 1), torch.zeros(3, D, dtype=torch.int64), torch.zeros(D), np.zeros((3, D), np.float32), torch.zeros(0, D)):
        with pytest.raises(ValueError):
            pkg.latent_classes(m, z)
    assert ops.calls == [] and made == []


def test_prior_latents_and_generate_on_stand_ins():
    pkg = load_package()
    ops = hl.latent_fake_ops()
    m = hl.set_apart(make_model(64, 8, ops=ops))
    Z, rows = 8, 6
    ops.calls.clear()
    z, comps = pkg.prior_latents(m, rows, rhythm=1, note=[0, 1, 0, 1, 1, 0], key=14, temperature=0.7, seed=5, offset=2)
    assert ops.calls == ["latent_draw"] and z.shape == (rows, 2 * Z + 24) and z.dtype == torch.float32 and comps.shape == (rows, 2) and comps.dtype == torch.int32
    assert comps.tolist() == [[1, k] for k in (0, 1, 0, 1, 1, 0)]
    want = torch.zeros(rows, 24)
    want[:, 14] = 1.0
    assert torch.equal(z[:, 2 * Z:], want)
    for s, e in enumerate("rn"):          # stream 0 is the rhythm latent, stream 1 the note latent
        ref = hl.draw_ref(getattr(m, "mu_%s_lookup" % e).weight.data.numpy(), getattr(m, "logvar_%s_lookup" % e).weight.data.numpy(), rows, s, 5, 2, 0.7,
                          comps[:, s].numpy())
        hl.check_draw(ref, z[:, s * Z:(s + 1) * Z].numpy(), tag=e)
    # drawn components; a row's numbers do not depend on the number of rows; chroma rows pass through
    ch = torch.rand(rows, 24)
    z6, c6 = pkg.prior_latents(m, rows, chroma=ch, seed=5)
    z2, c2 = pkg.prior_latents(m, 2, chroma=ch[0], seed=5)
    assert torch.equal(z6[:2, :2 * Z], z2[:, :2 * Z]) and torch.equal(c6[:2], c2) and torch.equal(z6[:, 2 * Z:], ch) and torch.equal(z2[:, 2 * Z:], ch[:1].expand(2, 24))
    assert not torch.equal(pkg.prior_latents(m, rows, key=0, seed=6)[0], pkg.prior_latents(m, rows, key=0, seed=5)[0])
    assert not torch.equal(pkg.prior_latents(m, rows, key=0, seed=5, offset=1)[0], pkg.prior_latents(m, rows, key=0, seed=5)[0])
    # temperature 0: the component means
    z0, c0 = pkg.prior_latents(m, rows, key=0, temperature=0, rhythm=np.array([0, 1, 1, 0, 0, 1]))
    assert torch.equal(z0[:, :Z], m.mu_r_lookup.weight.data[c0[:, 0].long()]) and torch.equal(z0[:, Z:2 * Z], m.mu_n_lookup.weight.data[c0[:, 1].long()])
    # generate is the decode of the z it returns, whichever decode
    was = m.training
    for kw, dec in ((dict(), lambda zz: pkg.greedy_decode(m, zz, 9, want_logp=False)[1]),
                    (dict(sample=dict(seed=1, temperature=0.9)), lambda zz: pkg.sample_decode(m, zz, 9, want_logp=False, seed=1, temperature=0.9)[1]),
                    (dict(beam=dict(width=2)), lambda zz: pkg.beam_decode(m, zz, 9, width=2)[0][:, 0]),
                    (dict(prompt=[5, 6]), lambda zz: pkg.continue_from(m, zz, torch.tensor([[5, 6]]).expand(rows, 2), 9, want_logp=False)[1])):
        ops.calls.clear()
        tok, zz, cc = pkg.generate(m, rows, steps=9, rhythm=0, key=3, seed=11, **kw)
        assert ops.calls.count("latent_draw") == 1 and tok.shape == (rows, 9) and tok.dtype == torch.int32 and m.training == was
        zp, cp = pkg.prior_latents(m, rows, rhythm=0, key=3, seed=11)
        assert torch.equal(zz, zp) and torch.equal(cc, cp) and torch.equal(tok, dec(zz)), kw


def test_mix_latents_and_morph_on_stand_ins(monkeypatch):
    pkg = load_package()
    from music_fader_nets_amd import decode
    ops = hl.latent_fake_ops()
    m = make_model(64, 8, ops=ops)
    Z, n = 8, 3
    D = 2 * Z + 24
    g = torch.Generator().manual_seed(3)
    za, zb = torch.randn(n, D, generator=g), torch.randn(n, D, generator=g)
    ops.calls.clear()
    z, om = pkg.mix_latents(m, za, zb, [0.0, 0.25, 0.5, 1.0])
    assert ops.calls == ["latent_mix"] and z.shape == (n, 4, D) and om.shape == (n, 2) and bool((om > 0).all())
    assert torch.equal(z[:, 0], za) and torch.equal(z[:, 3], zb)
    assert torch.equal(z[:, 1, 2 * Z:], za[:, 2 * Z:]) and torch.equal(z[:, 2, 2 * Z:], zb[:, 2 * Z:])          # the chroma steps at 0.5
    hl.check_mix(za.numpy(), zb.numpy(), [0.0, 0.25, 0.5, 1.0], hl.std_segs(Z), z.reshape(n * 4, D).numpy())
    zl, ol = pkg.mix_latents(m, za, zb, np.array([[0.5], [0.25], [2.0]]), mode="lerp", per_pair=True)
    assert bool((ol == 0).all()) and torch.allclose(zl[1, 0, :2 * Z], 0.25 * zb[1, :2 * Z] + 0.75 * za[1, :2 * Z], atol=1e-6)
    assert torch.allclose(zl[2, 0, :2 * Z], 2.0 * zb[2, :2 * Z] - za[2, :2 * Z], atol=1e-5)
    # morph: one encode of 2n rows, one mix, one decode of n * P rows; its ends are the decodes of za and zb
    made = dict(encode=[], decode=[])
    enc = m.encode
    monkeypatch.setattr(m, "encode", lambda x: (made["encode"].append(x.shape[0]), enc(x))[1])
    for name in ("greedy_decode", "sample_decode", "beam_decode"):
        fn = getattr(decode, name)
        monkeypatch.setattr(decode, name, lambda mm, zz, *a, _fn=fn, **k: (made["decode"].append(zz.shape[0]), _fn(mm, zz, *a, **k))[1])
    rs = np.random.RandomState(11)
    xa, xb = torch.from_numpy(rs.randint(0, 342, (n, 20))), torch.from_numpy(rs.randint(0, 342, (n, 20)))
    ca, cb = torch.from_numpy(rs.rand(n, 24).astype(np.float32)), torch.from_numpy(rs.rand(n, 24).astype(np.float32))
    was = m.training
    for eps in (None, (torch.randn(2 * n, Z, generator=g), torch.randn(2 * n, Z, generator=g))):
        ops.calls.clear(), made["encode"].clear(), made["decode"].clear()
        tok, z, om = pkg.morph(m, xa, ca, xb, cb, points=3, steps=7, eps=eps)
        assert made == dict(encode=[2 * n], decode=[n * 3]) and ops.calls.count("latent_mix") == 1 and m.training == was
        assert tok.shape == (n, 3, 7) and tok.dtype == torch.int32 and z.shape == (n, 3, D) and om.shape == (n, 2)
        m.eval()
        dr, dn = enc(torch.cat([xa, xb]))
        m.train(was)
        zr, zn = (d.mean if eps is None else d.mean + d.stddev * e for d, e in zip((dr, dn), eps or (None, None)))
        zab = torch.cat([zr, zn, torch.cat([ca, cb])], 1)
        assert torch.equal(z[:, 0], zab[:n]) and torch.equal(z[:, 2], zab[n:])
        for p, rows in ((0, zab[:n]), (2, zab[n:])):
            assert torch.equal(tok[:, p], pkg.greedy_decode(m, rows.contiguous(), 7, want_logp=False)[1])
    tok9 = pkg.morph(m, xa, ca, xb, cb, t=[0.0, 0.1, 1.0], steps=7, mode="lerp", sample=dict(seed=2))[0]
    assert tok9.shape == (n, 3, 7)
    assert pkg.morph(m, xa, ca, xb, cb, points=1, steps=7)[1].shape == (n, 1, D)          # one point: t = 0, piece A


def test_latent_classes_is_approx_qy_x_in_float64():
    pkg = load_package()
    ops = hl.latent_fake_ops()
    m = hl.set_apart(make_model(64, 8, ops=ops))
    Z, K, rows = 8, 2, 64
    z, comps = pkg.prior_latents(m, rows, key=0, seed=3)
    ops.calls.clear()
    qr, qn, yr, yn = pkg.latent_classes(m, z)
    assert "latent_draw" not in ops.calls and "latent_mix" not in ops.calls and qr.shape == (rows, K)          # no kernel of its own: fn_latent_fwd and yr.shape == (rows,) and yr.dtype == torch.int32
    seen = []
    for s, (e, q, y) in enumerate((("r", qr, yr), ("n", qn, yn))):
        zz = z[:, s * Z:(s + 1) * Z].double().numpy()
        mu, lv = (getattr(m, "%s_%s_lookup" % (w, e)).weight.data.double().numpy() for w in ("mu", "logvar"))
        ll = np.stack([(-0.5 * ((zz - mu[k]) ** 2 / np.exp(lv[k]) + lv[k] + np.log(2 * np.pi))).sum(1) + np.log(1.0 / K) for k in range(K)], 1)      # gmm_model.py:194-218
        want = np.exp(ll - ll.max(1, keepdims=True))
        want /= want.sum(1, keepdims=True)
        assert np.abs(q.numpy() - want).max() <= 1e-5 and np.array_equal(y.numpy(), want.argmax(1))
        seen.append(float(np.minimum(want[:, 0], want[:, 1]).max()))
        assert (y.numpy() == comps[:, s].numpy()).mean() > 0.8          # 3 sigma apart: the drawn component is mostly the likelier one
    assert max(seen) > 1e-3, seen                                        # not all saturated: the comparison sees the softmax
    assert all(torch.equal(a, b) for a, b in zip(pkg.latent_classes(m, z[:, :2 * Z]), (qr, qn, yr, yn)))


def test_the_script_parses_and_fails_cleanly_without_a_gpu(tmp_path):
    script = os.path.join(ROOT, "generate_midi.py")
    cfg = os.path.join(ROOT, "tests", "golden", "gmm_model_config.json")
    p = subprocess.run([sys.executable, script, "--config", cfg, "--rows", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "OUT_DIR" in p.stderr and "Traceback" not in p.stderr
    p = subprocess.run([sys.executable, script, "--config", cfg, str(tmp_path / "out"), "--rhythm", "high"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--rhythm" in p.stderr and "Traceback" not in p.stderr
    if torch.cuda.is_available():
        return                                                                   # tests/test_gpu_latent_ops.py runs it for real
    p = subprocess.run([sys.executable, script, "--config", cfg, str(tmp_path / "out"), "--rows", "2", "--steps", "8", "--rhythm", "1", "--note", "0", "--key", "3",
                        "--temperature", "0.8", "--seed", "4"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "no GPU visible" in p.stderr and "Traceback" not in p.stderr and not os.path.exists(str(tmp_path / "out"))
