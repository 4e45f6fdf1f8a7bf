"""Latent disentanglement report (disentangle.py, the six fn_* entry points of csrc/disentangle.hip), CPU side: known answers and the planted structure
on the float64 restatement of tests/helpers_disentangle.py, the host twins in a stand-alone sanitizer build against the restatement on the case list,
the entry points' answers to bad arguments, and the Python layer on stand-in ops."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_disentangle as hd
from helpers import make_model
from mfn_import import ROOT, load_package


# ------------------------------------------------------------------------------------------------------------------------------
# 1. known answers on the restatement
# ------------------------------------------------------------------------------------------------------------------------------
def _mi_of(bz, bf):
    m = hd.mi_ref(hd.hist_ref(bz[None].astype(np.uint8), bf[None].astype(np.uint8)).reshape(1, 64, 64))
    return m["scores"][0], int(m["hits"][0]), m["mag"][0]


def test_full_factorial_design_has_zero_information():
    """every (bz, bf) cell filled equally often: every argument of the logarithm is exactly 1"""
    for nz, nf, rep in ((4, 3, 5), (20, 20, 1), (64, 64, 2), (1, 7, 3)):
        bz, bf = np.repeat(np.arange(nz), nf * rep), np.tile(np.arange(nf), nz * rep)
        (I, hz, hf), hits, _ = _mi_of(bz, bf)
        assert I == 0.0 and abs(hz - np.log(nz)) <= 16 * hd.ULP * np.log(max(nz, 2)) and abs(hf - np.log(nf)) <= 16 * hd.ULP * np.log(nf), (nz, nf, I, hz, hf)
        assert hits == nz * rep


def test_bijection_of_a_discrete_factor_carries_its_entropy():
    g = np.random.default_rng(0)
    f = g.integers(0, 7, 500)
    f[:7] = np.arange(7)
    z = (np.array([3, 0, 6, 1, 5, 2, 4]) * 2.0)[f].astype(np.float32)[:, None]          # a bijection, spread over 13 of 20 bins
    lo, hi, _ = hd.range_ref(z)
    bz, _ = hd.bin_ref(z, lo, hi, 20)
    (I, hz, hf), hits, mag = _mi_of(bz[0], f)
    assert abs(I - hf) <= (hd.K_I + hd.K_H) * hd.ULP * (mag[0] + mag[2]) and abs(hz - hf) <= 2 * hd.K_H * hd.ULP * mag[2] and hits == 500


def test_constant_column_bin_zero_and_no_information():
    z = np.full((50, 1), 0.75, np.float32)
    lo, hi, st = hd.range_ref(z)
    bz, _ = hd.bin_ref(z, lo, hi, 20)
    assert lo[0] == hi[0] == np.float32(0.75) and st[0] == 0 and not bz.any()
    (I, hz, _), _, _ = _mi_of(bz[0], np.arange(50) % 5)
    assert I == 0.0 and hz == 0.0


def test_values_on_the_edges_land_in_the_stated_bins():
    """lo -> 0, hi -> bins - 1, an interior edge k -> bin k (the upper bin), just below it -> k - 1"""
    for bins in (1, 2, 20, 64):
        edges = np.arange(bins + 1, dtype=np.float32)
        below = np.nextafter(edges[1:], np.float32(0)).astype(np.float32)
        z = np.concatenate([edges, below])[:, None]
        lo, hi, _ = hd.range_ref(z)
        b, _ = hd.bin_ref(z, lo, hi, bins)
        assert lo[0] == 0 and hi[0] == bins
        assert b[0, :bins + 1].tolist() == list(range(bins)) + [bins - 1] and b[0, bins + 1:].tolist() == list(range(bins)), bins
    # a discrete factor: the level itself; what is no level is flagged
    f = np.array([[0.0], [2.0], [1.0], [2.5], [3.0], [-1.0]], np.float32)
    b, bad = hd.bin_ref(f[:3], None, None, 20, [3])
    assert b[0].tolist() == [0, 2, 1] and bad[0] == 0
    assert all(hd.bin_ref(f[[0, k]], None, None, 20, [3])[1][0] == 2 for k in (3, 4, 5))
    # a zero of either sign is one value for the range
    lo, hi, _ = hd.range_ref(np.array([[-0.0], [0.0]], np.float32))
    assert lo.tobytes() == hi.tobytes() == np.float32(0.0).tobytes()
    lo, hi, st = hd.range_ref(np.array([[1.0, np.nan], [np.inf, 2.0], [-3.0, 2.0]], np.float32))
    assert lo.tolist() == [-3.0, 2.0] and hi.tolist() == [1.0, 2.0] and st.tolist() == [1, 1]


def test_ranks_known_answers():
    for N in (1, 2, 7, 64):
        assert hd.ranks_ref(np.full((N, 1), 3.0, np.float32))[0].tolist() == [(N + 1) / 2] * N
    col = np.array([0.0, -0.0, 1.0, -1.0, 0.0], np.float32)
    assert hd.ranks_ref(col[:, None])[0].tolist() == [3.0, 3.0, 5.0, 1.0, 3.0]          # -0.0 ties 0.0
    g = np.random.default_rng(1)
    x = (np.round(g.standard_normal((300, 3)) * 3) / 3).astype(np.float32)
    r = hd.ranks_ref(x)
    for c in range(3):
        assert r[c].tobytes() == hd.ranks_by_definition(x[:, c]).tobytes()
        assert r[c].sum() == 300 * 301 / 2
    # the mutations are mutations
    assert not np.array_equal(hd.ranks_ref(x, le=True), r) and not np.array_equal(hd.ranks_ref(x, tie_once=True), r)


def test_rho_of_a_strictly_increasing_function_is_one():
    g = np.random.default_rng(2)
    for N in (2, 65, 1000):
        x = g.standard_normal(N).astype(np.float32)
        y = np.exp(x.astype(np.float64) / 4).astype(np.float32)
        assert len(set(x.tolist())) == N and len(set(y.tolist())) == N
        rk = hd.corr_ref(hd.ranks_ref(x[:, None]).T, hd.ranks_ref(y[:, None]).T)
        rho = rk["cross"][0, 0] / np.sqrt(rk["ss_x"][0] * rk["ss_y"][0])
        # the ranks are equal, so the three sums are the same sum up to the order-free rounding of each: 3 sums and a square root
        assert abs(rho - 1.0) <= 4 * hd.corr_k(N)["cross"] * hd.ULP, (N, rho)


def test_row_permutation_leaves_counts_and_rank_multisets():
    c = hd.cases()[6]
    z, f = hd.views(c)
    r = hd.reference(c)
    perm = np.random.default_rng(3).permutation(c["N"])
    lo, hi, _ = hd.range_ref(z[perm])
    assert lo.tobytes() == r["lo_z"].tobytes() and hi.tobytes() == r["hi_z"].tobytes()
    bz, _ = hd.bin_ref(z[perm], lo, hi, c["bins"])
    bf, _ = hd.bin_ref(f[perm], r["lo_f"], r["hi_f"], c["bins"], c["card"])
    assert np.array_equal(hd.hist_ref(bz, bf), r["counts"])
    assert np.array_equal(hd.ranks_ref(z[perm]), r["rk_z"][:, perm])


# ------------------------------------------------------------------------------------------------------------------------------
# 2. planted structure on the restatement
# ------------------------------------------------------------------------------------------------------------------------------
def test_planted_structure_on_the_restatement():
    worst = {}
    for seed in range(6):
        z, f, card = hd.planted(seed)
        fig = hd.check_planted(hd.figures_ref(z, f, card, 20), "seed %d" % seed)
        for k, v in fig.items():
            worst[k] = min(worst.get(k, v), v) if k in ("mi_1", "mi_3", "mig_f1") else max(worst.get(k, v), v)
    print("planted structure, worst over the seeds: %s; the bias (bins - 1)^2 / 2N = %.3f" % (worst, 19 * 19 / 4096))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the host twins in a stand-alone sanitizer build
# ------------------------------------------------------------------------------------------------------------------------------
def _run(exe, fin, fout, blob):
    with open(fin, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    return open(fout, "rb").read()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    tmp = tmp_path_factory.mktemp("disentangle")
    src = os.path.join(ROOT, "music-fader-nets_amd", "csrc", "host", "disentangle_check.cpp")
    exe = str(tmp / "disentangle_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror", src,
                    "-o", exe], check=True, capture_output=True, timeout=300)
    return lambda blob: _run(exe, str(tmp / "in.bin"), str(tmp / "out.bin"), blob)


def test_host_twins_against_the_restatement(twin):
    be = hd.TwinBackend(twin)
    worst, told = {}, set()
    for c in hd.cases():
        o = hd.run_pipeline(c, be)
        for k, v in hd.check_pipeline(c, o).items():
            worst[k] = max(worst.get(k, 0.0), v)
        for name, (key, arr) in hd.mutants(c).items():
            got = o[key][:, :c["N"]] if key != "counts" else o[key]
            if not np.array_equal(got, arr):
                told.add(name)
    print("twins: worst share of the fp64 bounds %s" % {k: round(v, 3) for k, v in worst.items()})
    assert told == set(hd.mutants(hd.cases()[0])), told


def test_host_twins_on_the_planted_structure(twin):
    be = hd.TwinBackend(twin)
    z, f, card = hd.planted(0)
    c = dict(tag="planted", N=2048, D=6, A=2, bins=20, card=card, zbuf=z, fbuf=f, off_z=0, off_f=0, n_pad=2048)
    o = hd.run_pipeline(c, be)
    hd.check_pipeline(c, o)
    sc = o["scores"].reshape(6, 2, 3)
    r = o["raw"][4] / np.sqrt(o["raw"][1][:, None] * o["raw"][3][None, :])
    rho = o["rk"][4] / np.sqrt(o["rk"][1][:, None] * o["rk"][3][None, :])
    hd.check_planted(dict(mi=sc[:, :, 0], h_factor=sc[0, :, 2], r2=r * r, rho=rho, accuracy=o["hits"].reshape(6, 2) / 2048), "twin")


def test_host_twins_flag_what_is_not_a_number_or_a_level(twin):
    be = hd.TwinBackend(twin)
    x = np.arange(24, dtype=np.float32).reshape(8, 3)
    x[2, 0], x[5, 2] = np.nan, -np.inf
    lo, hi, st = be.range(x, 0, 3)
    rl, rh, rs = hd.range_ref(x)
    assert st.tolist() == [1, 0, 1] == rs.tolist() and lo.tobytes() == rl.tobytes() and hi.tobytes() == rh.tobytes()
    img, st2 = be.bins(x, 0, 3, lo, hi, 20, None, 8, st)
    assert np.array_equal(img, hd.bin_ref(x, rl, rh, 20)[0]) and st2.tolist() == [1, 0, 1] and img[0, 2] == 0 and img[2, 5] == 0
    f = np.array([[0, 1], [1, 5], [2, 0.5], [1, np.nan]], np.float32)
    img, st = be.bins(f, 0, 2, np.zeros(2, np.float32), np.ones(2, np.float32), 4, [3, 6], 4, np.zeros(2, np.int32))
    assert st.tolist() == [0, 2] and img.tolist() == [[0, 1, 2, 1], [1, 5, 0, 0]]


def test_host_twin_answers_to_bad_sizes(twin):
    rc = lambda blob: int(np.frombuffer(twin(blob)[:4], np.int32)[0])
    f32 = lambda n: np.zeros(max(n, 0), np.float32).tobytes()
    #          N  P  ld
    for (N, P, ld), want in (((0, 2, 2), -2), ((3, 0, 2), -2), ((3, 2, 1), -2), ((3, 4097, 4097), -6), (((1 << 22) + 1, 1, 1), -6)):
        n = (N - 1) * ld + P if N > 0 and P > 0 else 0
        assert rc(hd._i32(0, N, P, ld) + f32(n)) == want, (N, P, ld)
        assert rc(hd._i32(3, N, P, ld, max(N, 1)) + f32(n)) == want, (N, P, ld)
    assert rc(hd._i32(3, 3, 2, 2, 2) + f32(6)) == -2                                      # n_pad < N
    #          N  P  ld bins n_pad card
    for (N, P, ld, bins, n_pad, card), want in (((3, 2, 2, 0, 3, None), -2), ((3, 2, 2, 65, 3, None), -6), ((3, 2, 2, 4, 2, None), -2), ((3, 2, 2, 4, 3, [0, 65]), -2),
                                                ((3, 2, 2, 4, 3, [-1, 0]), -2), ((3, 17, 17, 4, 3, [0] * 17), -6)):
        blob = hd._i32(1, N, P, ld, bins, n_pad, 0 if card is None else 1) + f32((N - 1) * ld + P) + f32(2 * P)
        assert rc(blob + (b"" if card is None else np.array(card, np.int32).tobytes())) == want, (N, P, ld, bins, n_pad, card)
    for (N, D, A, ldz, ldf), want in (((0, 1, 1, 4, 4), -2), ((4, 0, 1, 4, 4), -2), ((4, 1, 0, 4, 4), -2), ((4, 1, 1, 3, 4), -2), ((4, 1, 1, 4, 3), -2), ((4, 1, 17, 4, 4), -6)):
        nz, nf = ((D - 1) * ldz + N if D > 0 and N > 0 else 0), ((A - 1) * ldf + N if A > 0 and N > 0 else 0)
        assert rc(hd._i32(2, N, D, A, ldz, ldf) + bytes(nz) + bytes(nf)) == want, (N, D, A, ldz, ldf)
    for (N, P, Q, xrs, xcs, yrs, ycs), want in (((0, 1, 1, 1, 1, 1, 1), -2), ((2, 0, 1, 1, 1, 1, 1), -2), ((2, 1, 0, 1, 1, 1, 1), -2), ((2, 1, 1, 0, 1, 1, 1), -2),
                                                ((2, 1, 1, 1, 1, 1, 0), -2), ((2, 1, 17, 17, 1, 17, 1), -6)):
        nx = (N - 1) * xrs + (P - 1) * xcs + 1 if N > 0 and P > 0 else 0
        ny = (N - 1) * yrs + (Q - 1) * ycs + 1 if N > 0 and Q > 0 else 0
        assert rc(hd._i32(4, N, P, Q, xrs, xcs, yrs, ycs) + f32(nx) + f32(ny)) == want, (N, P, Q)
    assert rc(hd._i32(5, 0)) == -2


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the ABI without a GPU
# ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_argument_errors_without_gpu():
    load_package()
    from music_fader_nets_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "fadernets.h")).read()
    for name, text in (("FN_DIS_MAX_N", "(1 << 22)"), ("FN_DIS_MAX_D", "4096"), ("FN_DIS_MAX_A", "16"), ("FN_DIS_MAX_BINS", "64"), ("FN_DIS_RANGE_CHUNK", "1024"),
                       ("FN_DIS_HIST_CHUNK", "4096"), ("FN_DIS_RANK_ROWS", "1024"), ("FN_DIS_RANK_TILE", "1024"), ("FN_DIS_NONFINITE", "1"),
                       ("FN_DIS_BAD_LEVEL", "2"), ("FN_DIS_MI_COLS", "3")):
        assert re.search(r"^#define %s\s+%s(\s|$)" % (name, re.escape(text)), hdr, re.M) and eval(text) == getattr(_lib, name), name
    assert hd.HIST_CHUNK == _lib.FN_DIS_HIST_CHUNK and lib.fn_version() == 6
    assert {"fn_column_range", "fn_bin_columns", "fn_joint_hist", "fn_column_ranks", "fn_column_corr", "fn_mi_scores"} <= set(_lib.SIGNATURES)
    assert "disentangle" not in open(os.path.join(ROOT, "include", "fadernets_host.h")).read()          # the twins live in the stand-alone driver only
    buf = (C.c_int32 * 4096)()
    at = (C.addressof(buf) + 15) // 16 * 16
    odd, odd4 = at + 2, at + 4
    big = (1 << 22) + 1

    def rng(x=at, ld=4, N=8, P=3, lo=at, hi=at, status=at):
        return lib.fn_column_range(x, ld, N, P, lo, hi, status, None)

    for k in ("x", "lo", "hi", "status"):
        assert rng(**{k: None}) == -1 and rng(**{k: odd}) == -3, k
    for kw in (dict(N=0), dict(N=-1), dict(P=0), dict(ld=2)):
        assert rng(**kw) == -2, kw
    assert rng(N=big) == -6 and rng(P=4097, ld=4097) == -6 and rng(x=None, N=0) == -1 and rng(N=0, P=4097, ld=4097) == -2 and rng(N=big, lo=odd) == -6

    def bins(x=at, ld=4, N=8, P=3, lo=at, hi=at, card=None, bins=20, img=at, n_pad=8, status=at):
        arr = None if card is None else (C.c_int32 * len(card))(*card)
        return lib.fn_bin_columns(x, ld, N, P, lo, hi, arr, bins, img, n_pad, status, None)

    for k in ("x", "lo", "hi", "img", "status"):
        assert bins(**{k: None}) == -1, k
    for k in ("x", "lo", "hi", "status"):
        assert bins(**{k: odd}) == -3, k
    for kw in (dict(N=0), dict(P=0), dict(ld=2), dict(bins=0), dict(bins=-1), dict(n_pad=7), dict(card=[0, 65, 0]), dict(card=[0, 0, -1])):
        assert bins(**kw) == -2, kw
    for kw in (dict(N=big, n_pad=big), dict(P=4097, ld=4097), dict(bins=65), dict(P=17, ld=17, card=[0] * 17)):
        assert bins(**kw) == -6, kw
    assert bins(x=None, bins=0) == -1 and bins(bins=0, P=4097, ld=4097) == -2 and bins(bins=65, x=odd) == -6

    def hist(bz=at, ldz=8, D=2, bf=at, ldf=8, A=2, N=8, counts=at):
        return lib.fn_joint_hist(bz, ldz, D, bf, ldf, A, N, counts, None)

    for k in ("bz", "bf", "counts"):
        assert hist(**{k: None}) == -1, k
    assert hist(counts=odd) == -3
    for kw in (dict(N=0), dict(D=0), dict(A=0), dict(ldz=7), dict(ldf=7)):
        assert hist(**kw) == -2, kw
    for kw in (dict(N=big, ldz=big, ldf=big), dict(D=4097), dict(A=17)):
        assert hist(**kw) == -6, kw
    assert hist(bz=None, N=0) == -1 and hist(N=0, A=17) == -2 and hist(A=17, counts=odd) == -6

    def ranks(x=at, ld=4, N=8, P=3, r=at, n_pad=8):
        return lib.fn_column_ranks(x, ld, N, P, r, n_pad, None)

    for k in ("x", "r"):
        assert ranks(**{k: None}) == -1 and ranks(**{k: odd}) == -3, k
    for kw in (dict(N=0), dict(P=0), dict(ld=2), dict(n_pad=7)):
        assert ranks(**kw) == -2, kw
    assert ranks(N=big, n_pad=big) == -6 and ranks(P=4097, ld=4097) == -6 and ranks(N=0, x=None) == -1 and ranks(n_pad=7, P=4097, ld=4097) == -2

    def corr(X=at, xrs=4, xcs=1, P=3, Y=at, yrs=2, ycs=1, Q=2, N=8, mx=at, sx=at, my=at, sy=at, cr=at):
        return lib.fn_column_corr(X, xrs, xcs, P, Y, yrs, ycs, Q, N, mx, sx, my, sy, cr, None)

    for k in ("X", "Y", "mx", "sx", "my", "sy", "cr"):
        assert corr(**{k: None}) == -1 and corr(**{k: odd}) == -3, k
    for k in ("mx", "sx", "my", "sy", "cr"):
        assert corr(**{k: odd4}) == -3, k          # doubles: 8-byte aligned
    for kw in (dict(N=0), dict(P=0), dict(Q=0), dict(xrs=0), dict(xcs=0), dict(yrs=0), dict(ycs=-1)):
        assert corr(**kw) == -2, kw
    for kw in (dict(N=big), dict(P=4097), dict(Q=17)):
        assert corr(**kw) == -6, kw
    assert corr(X=None, N=0) == -1 and corr(N=0, Q=17) == -2 and corr(Q=17, cr=odd) == -6

    def mi(counts=at, pairs=2, out=at, hits=at):
        return lib.fn_mi_scores(counts, pairs, out, hits, None)

    for k in ("counts", "out", "hits"):
        assert mi(**{k: None}) == -1 and mi(**{k: odd}) == -3, k
    assert mi(out=odd4) == -3 and mi(pairs=0) == -2 and mi(pairs=-1) == -2 and mi(pairs=65537) == -6 and mi(pairs=0, out=None) == -1


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the Python layer on stand-ins
# ------------------------------------------------------------------------------------------------------------------------------
LAUNCHES = ["column_range"] * 2 + ["bin_columns"] * 2 + ["joint_hist", "mi_scores"] + ["column_ranks"] * 2 + ["column_corr"] * 2


def _count_copies(monkeypatch):
    from music_fader_nets_amd import disentangle as mod
    n, real = [0], mod._to_host

    def counted(t):
        n[0] += 1
        return real(t)

    monkeypatch.setattr(mod, "_to_host", counted)
    return n


def test_disentanglement_on_stand_ins(monkeypatch):
    """the launches, the single host copy, and every figure against its definition on the restatement's matrices"""
    pkg = load_package()
    ops = hd.dis_fake_ops()
    copies = _count_copies(monkeypatch)
    z, f, card = hd.planted(0)
    wide = torch.from_numpy(np.concatenate([np.zeros((2048, 1), np.float32), z, np.ones((2048, 2), np.float32)], 1))
    res = pkg.disentanglement(wide[:, 1:7], torch.from_numpy(f), card=card, bins=20, names=["f0", "f1"], ops=ops)
    assert ops.calls == LAUNCHES and copies[0] == 1
    fig = hd.figures_ref(z, f, card, 20)
    assert np.array_equal(res.mi, fig["mi"]) and np.array_equal(res.h_factor, fig["h_factor"]) and np.array_equal(res.h_code, fig["h_code"])
    assert np.allclose(res.r2[:, 0], fig["r2"][:, 0], rtol=1e-13) and np.allclose(res.rho[:, 0], fig["rho"][:, 0], rtol=1e-13)
    assert np.isnan(res.r2[:, 1]).all() and np.isnan(res.rho[:, 1]).all() and np.isnan(res.accuracy[:, 0]).all()
    assert np.array_equal(res.accuracy[:, 1], fig["accuracy"][:, 1])
    hd.check_planted(dict(mi=res.mi, h_factor=res.h_factor, r2=np.where(np.isnan(res.r2), 0, res.r2), rho=np.where(np.isnan(res.rho), 0, res.rho),
                          accuracy=np.where(np.isnan(res.accuracy), 0, res.accuracy)))
    top = lambda col: np.sort(col)[-1] - np.sort(col)[-2]
    assert np.allclose(res.mig, [top(fig["mi"][:, a]) / fig["h_factor"][a] for a in range(2)], rtol=1e-14)
    assert np.allclose(res.sap, [top(fig["r2"][:, 0]), top(fig["accuracy"][:, 1])], rtol=1e-12)
    sq = fig["mi"] ** 2
    assert np.allclose(res.modularity, 1 - (sq.sum(1) - sq.max(1)) / sq.max(1), rtol=1e-13)
    assert res.winner["mi"].tolist() == [1, 5] and res.winner["r2"].tolist() == [3, -1] and res.winner["rho"].tolist() == [1, -1]
    assert res.interpretability[0] == res.r2[:, 0].max() and np.isnan(res.interpretability[1]) and res.names == ["f0", "f1"] and res.card == [0, 3] and res.n == 2048
    # all factors discrete: no rank and no correlation launch
    ops.calls.clear()
    r1 = pkg.disentanglement(torch.from_numpy(z), torch.from_numpy(f[:, 1]), card=[3], ops=ops)
    assert ops.calls == LAUNCHES[:6] and np.isnan(r1.rho).all() and np.array_equal(r1.mi[:, 0], res.mi[:, 1]) and (r1.modularity == 1).all()


def test_degenerate_cases_have_their_documented_values():
    pkg = load_package()
    ops = hd.dis_fake_ops()
    z, f, card = hd.planted(1, N=300)
    t = torch.from_numpy
    one = pkg.disentanglement(t(z[:, 3]), t(f), card=card, ops=ops)                          # D == 1: the runner-up is 0
    assert one.mi.shape == (1, 2) and np.array_equal(one.mig, one.mi[0] / one.h_factor) and one.sap[0] == one.r2[0, 0] and one.sap[1] == one.accuracy[0, 1]
    assert one.winner["mi"].tolist() == [0, 0]
    const = np.stack([f[:, 0], np.full(300, 2.0, np.float32)], 1)
    res = pkg.disentanglement(t(z), t(const), ops=ops)                                        # a constant factor
    assert res.h_factor[1] == 0 and np.isnan(res.mig[1]) and not np.isnan(res.mig[0]) and (res.r2[:, 1] == 0).all() and (res.rho[:, 1] == 0).all() and res.sap[1] == 0
    zc = z.copy()
    zc[:, 2] = -1.5                                                                           # a constant code column: no information, modularity NaN
    res = pkg.disentanglement(t(zc), t(f), card=card, ops=ops)
    assert (res.mi[2] == 0).all() and np.isnan(res.modularity[2]) and res.r2[2, 0] == 0 and res.rho[2, 0] == 0 and res.h_code[2] == 0
    assert pkg.disentanglement(t(z), t(f[:, 0]), ops=ops).modularity.tolist() == [1.0] * 6   # A == 1
    assert pkg.disentanglement(t(z[:1]), t(f[:1]), card=card, bins=1, ops=ops).mi.tolist() == [[0.0, 0.0]] * 6          # N == 1


def test_python_value_errors():
    pkg = load_package()
    ops = hd.dis_fake_ops()
    z, f, card = hd.planted(2, N=64)
    t = torch.from_numpy
    ok = dict(codes=t(z), factors=t(f), card=card, bins=20, names=None)
    for kw in (dict(codes=z), dict(codes=None), dict(codes=t(z).double()), dict(codes=t(z)[:0]), dict(codes=t(z)[None]), dict(codes=torch.zeros(2, 4097)),
               dict(factors=t(f)[:63]), dict(factors=f), dict(factors=t(f).long()), dict(factors=torch.zeros(64, 17)), dict(card=[0]), dict(card=[0, 65]),
               dict(card=[0, -1]), dict(card=[0, 2.0]), dict(card=[0, True]), dict(card=3), dict(bins=0), dict(bins=65), dict(bins=2.0), dict(bins=True),
               dict(bins=None), dict(names=["a"]), dict(names="ab"), dict(names=[1, 2])):
        with pytest.raises(ValueError):
            pkg.disentanglement(ops=ops, **dict(ok, **kw))
    assert ops.calls == []
    # what the status words report, naming the column
    for r, c, v, text in ((5, 2, np.nan, "codes: column 2 "), (0, 4, np.inf, "codes: column 4 ")):
        bad = z.copy()
        bad[r, c] = v
        with pytest.raises(ValueError, match=text):
            pkg.disentanglement(t(bad), t(f), card=card, ops=ops)
    bad = f.copy()
    bad[7, 1] = 3.0
    with pytest.raises(ValueError, match=r"factors: column 1 \(lvl\) holds a value that is not an integer in \[0, 3\)"):
        pkg.disentanglement(t(z), t(bad), card=card, names=["dens", "lvl"], ops=ops)
    bad[7, 1], bad[9, 0] = 1.0, -np.inf
    with pytest.raises(ValueError, match=r"factors: column 0 \(dens\) holds a NaN or an infinity"):
        pkg.disentanglement(t(z), t(bad), card=card, names=["dens", "lvl"], ops=ops)
    with pytest.raises(ValueError):
        pkg.disentanglement_report(torch.nn.Linear(2, 2), [])
    m = make_model(64, 8, ops=ops)
    for kw in (dict(bins=0), dict(extra=3)):
        with pytest.raises(ValueError):
            pkg.disentanglement_report(m, [], **kw)
    with pytest.raises(RuntimeError):
        pkg.disentanglement_report(m, [])
    from music_fader_nets_amd.epochs import evaluation_phase
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError):
            evaluation_phase(None, [], disentangle=bad)


def _loaders(pkg, rs, sizes=(5, 5, 5), T=20):
    from music_fader_nets_amd.synth import synth_batch
    out = []
    for B in sizes:
        b = synth_batch(rs, B, T, 8)
        out.append((b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"]))
    return out


def test_disentanglement_report_on_stand_ins(monkeypatch):
    """one encode per batch, the codes are the concatenated encode means, no host copy but the one, extra factors"""
    pkg = load_package()
    ops = hd.dis_fake_ops()
    m = make_model(64, 4, ops=ops)
    copies = _count_copies(monkeypatch)
    dl = _loaders(pkg, np.random.RandomState(5))
    ops.calls.clear(), ops.seen.clear()
    rep = pkg.disentanglement_report(m, dl, bins=8)
    assert [s for s in ops.seen] == [(None, 4, 5)] * 3 and copies[0] == 1 and [c for c in ops.calls if c in LAUNCHES] == LAUNCHES
    m.eval()
    means = torch.cat([torch.cat([d.mean for d in m.encode(torch.as_tensor(x[0]).long())], 1) for x in dl])
    assert rep.codes.shape == (15, 8) and torch.equal(rep.codes, means)
    dens = np.stack([np.concatenate([x[4] for x in dl]), np.concatenate([x[5] for x in dl])], 1).astype(np.float32)
    assert np.array_equal(rep.factors.numpy(), dens)
    res = pkg.disentanglement(rep.codes, rep.factors, bins=8, names=["r_density", "n_density"], ops=ops)
    for a, b in zip(rep.result[:9], res[:9]):
        assert np.array_equal(a, b, equal_nan=True)
    assert rep.fader_ok == all(res.winner[k].tolist() == [0, 4] for k in ("mi", "r2", "rho")) and rep.result.names == ["r_density", "n_density"]
    key = lambda x: (np.asarray(x[0])[:, 0] % 3, [3])
    rep2 = pkg.disentanglement_report(m, dl, bins=8, extra=key)
    assert rep2.result.card == [0, 0, 3] and rep2.result.mi.shape == (8, 3) and np.array_equal(rep2.result.mi[:, :2], rep.result.mi)
    assert np.array_equal(rep2.factors[:, 2].numpy(), np.concatenate([key(x)[0] for x in dl]).astype(np.float32))


def test_evaluation_phase_is_unchanged_without_disentangle_and_adds_one_line_with():
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch

    def run(**kw):
        ops = hd.dis_fake_ops()
        m = make_model(64, 4, ops=ops)
        tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
        rs = np.random.RandomState(8)
        loaders = [_loaders(pkg, rs, (4, 3), 12), []]
        b = synth_batch(rs, 3, 12, 8)
        loaders[1].append((b["d"], b["r"], b["n"], b["c"], b["a"], b["a"], b["r_density"], b["n_density"]))
        lines = []
        torch.manual_seed(4)
        res = pkg.evaluation_phase(tr, loaders, log=lines.append, step=20000, **kw)
        return lines, list(ops.calls), res

    base, off, on = run(), run(disentangle=False), run(disentangle=True)
    assert off[0] == base[0] and off[1] == base[1] and len(base[0]) == 6 and all("dis" not in r for r in off[2])
    assert not set(LAUNCHES) & set(base[1])
    assert len(on[0]) == 8 and [l for l in on[0] if not l.startswith("DIS: ")] == base[0]
    num = r"(-?\d[\d.e+-]*|nan)"
    for at, r in ((3, on[2][0]), (7, on[2][1])):
        assert re.fullmatch(r"DIS: r_density %s  %s  \d+  %s  %s  n_density %s  %s  \d+  %s  %s" % ((num,) * 8), on[0][at]), on[0][at]
        assert r["dis"].result.n == (7 if at == 3 else 3) and isinstance(r["dis"].fader_ok, bool)
