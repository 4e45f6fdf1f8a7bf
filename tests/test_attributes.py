"""Controllability metrics (attributes.py, fn_event_attributes / fn_sweep_scores), CPU side: the restatement of tests/helpers_attributes.py against
tests/golden/attributes.npz (the reference's piano-roll fill, attributes, classes and calculate_* methods, executed by the golden generator), the two
statements of the definition against each other, the host twin in a stand-alone sanitizer build, the answers of the entry points to bad arguments,
every ValueError of the Python layer, and controllability / evaluate through CPU stand-ins of the kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_attributes as ha
from helpers import make_model
from mfn_import import ROOT, load_package

GOLDEN = os.path.join(ROOT, "tests", "golden", "attributes.npz")


def _groups():
    g = np.load(GOLDEN)
    for grp in ("d", "w"):
        yield grp, g, dict(zip(ha.FIELDS, (int(x) for x in g[grp + "/params"])))


def _score_cases_of_the_fixture():
    g = np.load(GOLDEN)
    k = 0
    while "s%d/r" % k in g:
        P = "s%d/" % k
        which, r_std, n_std = g[P + "meta"]
        yield str(g[P + "tag"]), (g[P + "r"], g[P + "n"], g[P + "status"], g[P + "values"], int(which), float(r_std), float(n_std)), g[P + "scores"], int(g[P + "n_used"])
        k += 1


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the restatement against the reference's code
# ------------------------------------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_helper_generates():
    """the streams and score inputs in the fixture are the ones the helper builds (the fixture was not made from something else)"""
    for (grp, g, p), (g2, p2, names, tok) in zip(_groups(), ha.fixture_streams()):
        assert grp == g2 and p == p2 and np.array_equal(g[grp + "/tokens"], tok) and list(g[grp + "/names"]) == names
        assert tok.shape[1] == 100 and 8 <= tok.shape[0] <= 40
    cases = ha.score_cases() + [ha.unused_scores_case()]
    got = list(_score_cases_of_the_fixture())
    assert len(got) == len(cases) and sorted({c[1].shape[0] for c in cases}) == [1, 5, 67]
    for (tag, args, _, _), c in zip(got, cases):
        assert tag == c[0] and all(np.array_equal(a, b) for a, b in zip(args, c[1:]))
    assert os.path.getsize(GOLDEN) < 200 * 1024


@pytest.mark.parametrize("statement", [ha.attributes_sets, ha.attributes_words], ids=["sets", "words"])
def test_rows_reproduce_the_reference(statement):
    """rolls, rhythm, notes, n_cells and classes exact; densities equal as fp32"""
    seen = dict(rows=0, empty=0, c_r=set(), c_n=set(), hold=0, cleared=0)
    for grp, g, p in _groups():
        P = grp + "/"
        start = g[P + "roll_start"]
        for i, row in enumerate(g[P + "tokens"]):
            name = "%s %d %s" % (grp, i, g[P + "names"][i])
            a = statement(row, p)
            nc = int(g[P + "n_cells"][i])
            assert a["n_cells"] == nc and a["status"] == (0 if nc else ha.EMPTY), name
            roll = np.unpackbits(g[P + "roll"][start[i]:start[i + 1]], axis=1).astype(bool).reshape(nc, 128)
            assert np.array_equal(a["roll"], roll), name
            assert np.array_equal(a["rhythm"][:nc], g[P + "rhythm"][i, :nc]) and np.array_equal(a["notes"][:nc], g[P + "notes"][i, :nc]), name
            assert not a["rhythm"][nc:].any() and not a["notes"][nc:].any(), name
            assert (a["c_r"], a["c_n"]) == (int(g[P + "c_r"][i]), int(g[P + "c_n"][i])), name
            for k in ("r_density", "n_density"):
                assert a[k].dtype == np.float32 and a[k] == np.float32(g[P + k][i]), (name, k, a[k], g[P + k][i])
            seen["rows"] += 1
            seen["empty"] += nc == 0
            seen["c_r"].add(a["c_r"]), seen["c_n"].add(a["c_n"])
            seen["hold"] += int((a["rhythm"] == 2).sum())
        if grp == "w":
            used = np.unpackbits(g[P + "roll"], axis=1).astype(bool).any(0)
            assert all(used[32 * k:32 * k + 32].any() for k in range(4)) and used[0] and used[127]          # all four words of the pitch set
    assert seen["rows"] >= 40 and seen["empty"] >= 3 and seen["c_r"] == {0, 1, 2} and seen["c_n"] == {0, 1, 2} and seen["hold"] > 100, seen


def test_hand_rows_hit_the_clauses_they_are_named_for():
    p = ha.DEFAULT
    rows = ha.hand_rows()
    grid = lambda name: ha.grid_of(ha.tokens_to_notes(rows[name], p), p)
    cells = lambda name: np.flatnonzero(ha.attributes_sets(rows[name], p)["roll"][:, 40]).tolist()
    assert cells("same pitch back to back: the cleared cell") == [0, 2, 3]
    assert cells("a one-cell note that vanishes") == [1, 2, 3] and grid("a one-cell note that vanishes")[1][0] == (40, 0, 1)
    assert ha.tokens_to_notes(rows["re-strike while sounding"], p) == [(40, 0, 30), (40, 30, 60)]
    nc, placed = grid("a >= b: a kept note that fills nothing")
    assert nc == 8 and placed == [(40, 5, 4)] and not ha.attributes_sets(rows["a >= b: a kept note that fills nothing"], p)["roll"].any()
    nc, placed = grid("a == n_cells")
    assert placed[0][1] == nc == 8
    assert ha.tokens_to_notes(rows["note-off without a note-on"], p) == [(40, 20, 50)]
    assert ha.tokens_to_notes(rows["eos mid-row with notes behind it"], p) == [(40, 0, 50)]
    assert ha.tokens_to_notes(rows["one note never closed"], p) == [(40, 0, 130)]
    assert ha.tokens_to_notes(rows["zero-length notes are dropped"], p) == [(42, 30, 90)]
    assert ha.tokens_to_notes(rows["pad and velocity tokens between"], p) == [(40, 0, 75), (43, 50, 100)]


def test_scores_reproduce_the_reference():
    """against the reference's calculate_* with scikit-learn's LinearRegression: within 1e-8 (fp64 sums of fewer than 2^15 terms of magnitude about 10)"""
    worst, flat = 0.0, 0
    for tag, args, scores, n_used in _score_cases_of_the_fixture():
        ref = ha.sweep_scores_ref(*args)
        assert ref["n_used"] == n_used, tag
        if n_used == 0:
            assert all(np.isnan(ref[k]) for k in ha.SCORE_KEYS) and np.isnan(scores).all()
            continue
        d = max(abs(ref[k] - s) for k, s in zip(ha.SCORE_KEYS, scores))
        worst = max(worst, d)
        assert d <= 1e-8, (tag, d)
        flat += int(args[0].shape[0] == 1 and scores[2] == 1.0)               # S = 1: the one sample is the flat row, and its R2 is 1.0
    print("largest difference to the reference's scores: %.3e" % worst)
    assert flat == 2


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the definition, stated twice
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_two_statements_of_the_definition_agree():
    seen = dict(ok=0, empty=0, overflow=0)
    for c in ha.kernel_cases():
        a = ha.event_attributes_ref(c["tok"], c["steps"], c["p"], c["cells_ld"], ha.attributes_sets)
        b = ha.event_attributes_ref(c["tok"], c["steps"], c["p"], c["cells_ld"], ha.attributes_words)
        ha.same_attributes(a, b, c["tag"])
        for k, v in (("ok", 0), ("empty", ha.EMPTY), ("overflow", ha.OVERFLOW)):
            seen[k] += int((a["status"] == v).sum())
        if c["tag"] == "cells_ld 40 overflows":
            assert a["status"].tolist()[:5] == [0, ha.OVERFLOW, 0, ha.OVERFLOW, ha.OVERFLOW] and a["n_cells"].tolist()[:3] == [28, 60, 40]
            assert np.isnan(a["r_density"][1]) and a["c_r"][1] == -1 and not a["rhythm"][1].any()
        if c["tag"] == "1024 steps, 2048 cells":
            assert a["status"].tolist() == [0, 0, ha.OVERFLOW] and a["n_cells"][2] == 4 * (1023 * 100 // 50 + 1) and (a["n_cells"][:2] > 256).all()
        if c["tag"] == "n_pitch 200":
            wide = ha.event_attributes_ref(c["tok"], c["steps"], dict(c["p"], n_pitch=128), c["cells_ld"])
            ha.same_attributes(a, wide, c["tag"])
            assert (a["notes"].max(1) > 0).all()
        if c["tag"] == "vocab_size cuts every shift":
            assert (a["status"] == ha.EMPTY).all()                                       # the clock never moves: no note is kept
        if c["tag"] == "vocab_size cuts the ranges":
            full = ha.event_attributes_ref(c["tok"], c["steps"], dict(c["p"], vocab_size=0), c["cells_ld"])
            assert (a["n_cells"] > 0).all() and (a["n_cells"] < full["n_cells"]).all()
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the host twin in a stand-alone sanitizer build
# ------------------------------------------------------------------------------------------------------------------------------
def _run(exe, fin, fout, blob):
    with open(fin, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    return open(fout, "rb").read()


def test_host_twin_stand_alone_under_sanitizers(tmp_path):
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    src = os.path.join(ROOT, "music-fader-nets_amd", "csrc", "host", "attr_check.cpp")
    exe = str(tmp_path / "attr_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror", src, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for c in ha.kernel_cases():
        ref = ha.event_attributes_ref(c["tok"], c["steps"], c["p"], c["cells_ld"])
        rows, tok_ld = c["tok"].shape
        for cells in (1, 0):
            raw = _run(exe, fin, fout, np.array([0, rows, c["steps"], tok_ld, c["cells_ld"], cells, 0, 0], np.int32).tobytes()
                       + ha.params_bytes(c["p"]).tobytes() + np.ascontiguousarray(c["tok"]).tobytes())
            assert len(raw) == 4 + rows * 24 + 2 * cells * rows * c["cells_ld"] and np.frombuffer(raw[:4], np.int32)[0] == 0, c["tag"]
            body = raw[4:]
            got = {}
            for k in ("n_cells", "status", "r_density", "n_density", "c_r", "c_n"):
                got[k], body = np.frombuffer(body[:4 * rows], ha.OUT_DTYPES[k]), body[4 * rows:]
            if cells:
                got["rhythm"] = np.frombuffer(body[:rows * c["cells_ld"]], np.uint8).reshape(rows, -1)
                got["notes"] = np.frombuffer(body[rows * c["cells_ld"]:], np.uint8).reshape(rows, -1)
            ha.same_attributes(got, ref, c["tag"], cells=bool(cells))
    for tag, args, _, _ in _score_cases_of_the_fixture():
        r, n, status, values, which, r_std, n_std = args
        S, Vn = r.shape
        raw = _run(exe, fin, fout, np.array([1, S, Vn, which, 0, 0, 0, 0], np.int32).tobytes() + np.array([r_std, n_std]).tobytes() + values.tobytes()
                   + r.tobytes() + n.tobytes() + status.tobytes())
        assert len(raw) == 40 and np.frombuffer(raw[:4], np.int32)[0] == 0
        sc = np.frombuffer(raw[8:], np.float64)
        ha.same_scores(dict(zip(ha.SCORE_KEYS, sc), n_used=int(np.frombuffer(raw[4:8], np.int32)[0])), ha.sweep_scores_ref(*args), 1e-10, tag)
    # what the twin answers to bad sizes
    for hd, want in (([0, 1, 0, 4, 8, 0, 0, 0], -2), ([0, 1, 5, 4, 8, 0, 0, 0], -2)):
        raw = _run(exe, fin, fout, np.array(hd, np.int32).tobytes() + ha.params_bytes(ha.DEFAULT).tobytes() + np.zeros(4, np.int32).tobytes())
        assert np.frombuffer(raw, np.int32).tolist() == [want]


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the ABI without a GPU
# ------------------------------------------------------------------------------------------------------------------------------
def test_attribute_entry_points_argument_errors_without_gpu():
    load_package()
    from music_fader_nets_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "fadernets.h")).read()
    assert C.sizeof(_lib.FnAttrParams) == 48 == ha.PARAMS_DTYPE.itemsize and lib.fn_version() == 6
    for name in ("FN_ATTR_MAX_STEPS", "FN_ATTR_MAX_CELLS", "FN_ATTR_MAX_SAMPLES", "FN_ATTR_EMPTY", "FN_ATTR_OVERFLOW"):
        assert int(re.search(r"^#define %s (\d+)$" % name, hdr, re.M).group(1)) == getattr(_lib, name), name
    assert (_lib.FN_ATTR_MAX_STEPS, _lib.FN_ATTR_MAX_CELLS, _lib.FN_ATTR_EMPTY, _lib.FN_ATTR_OVERFLOW) == (ha.MAX_STEPS, ha.MAX_CELLS, ha.EMPTY, ha.OVERFLOW)
    assert hasattr(lib, "fn_event_attributes") and hasattr(lib, "fn_sweep_scores")
    buf = (C.c_int32 * 4096)()
    b = C.cast(buf, C.c_void_p)
    ok = dict(tokens=b, tok_ld=8, rows=2, steps=8, params=b, n_cells=b, status=b, r=b, n=b, c_r=b, c_n=b, rhythm=None, notes=None, cells_ld=64)
    order = ("tokens", "tok_ld", "rows", "steps", "params", "n_cells", "status", "r", "n", "c_r", "c_n", "rhythm", "notes", "cells_ld")
    call = lambda **kw: lib.fn_event_attributes(*[dict(ok, **kw)[k] for k in order], None)
    for k in ("tokens", "params", "n_cells", "status", "r", "n", "c_r", "c_n"):
        assert call(**{k: None}) == -1, k
    for kw in (dict(rows=0), dict(rows=-1), dict(steps=0), dict(steps=1025, tok_ld=1025), dict(cells_ld=0), dict(cells_ld=2049), dict(tok_ld=7)):
        assert call(**kw) == -2, kw
    assert call(tokens=None, rows=0) == -1                                     # null pointers are answered first
    ok = dict(r=b, n=b, status=b, S=4, Vn=8, values=b, which=0, r_std=1.0, n_std=1.0, scores=b, n_used=b)
    order = ("r", "n", "status", "S", "Vn", "values", "which", "r_std", "n_std", "scores", "n_used")
    call = lambda **kw: lib.fn_sweep_scores(*[dict(ok, **kw)[k] for k in order], None)
    for k in ("r", "n", "status", "values", "scores", "n_used"):
        assert call(**{k: None}) == -1, k
    for kw in (dict(S=0), dict(S=4097), dict(Vn=1), dict(Vn=65), dict(which=2), dict(which=-1)):
        assert call(**kw) == -2, kw


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the Python layer: every ValueError, before a launch; controllability and evaluate on stand-ins
# ------------------------------------------------------------------------------------------------------------------------------
def test_python_value_errors_come_before_any_launch():
    pkg = load_package()
    ops = ha.attr_fake_ops()
    tok = torch.zeros(3, 10, dtype=torch.int32)
    EV, EG = pkg.EventVocab, pkg.EventGrid
    assert EG() == (178, 100, 25, 2, 4)
    for kw in (dict(eos=-1), dict(eos=342), dict(eos=1.0), dict(eos=True), dict(eos=5), dict(eos=200), dict(vocab=None), dict(vocab=(2, 90)),
               dict(vocab=EV(2, 90, 0)), dict(vocab=EV(2, 90, 129)), dict(vocab=EV(2, 80, 88)), dict(vocab=EV(300, 90, 88)), dict(vocab=EV(2, 90, 89)),
               dict(grid=None), dict(grid=(178, 100)), dict(grid=EG(n_shift=0)), dict(grid=EG(shift_lo=300)), dict(grid=EG(shift_lo=100)),
               dict(grid=EG(ticks_num=0)), dict(grid=EG(ticks_den=257)), dict(grid=EG(beat_cells=65)), dict(grid=EG(ticks_num=2.5)), dict(want_cells=1)):
        with pytest.raises(ValueError):
            pkg.event_attributes(tok, ops=ops, **kw)
    for bad in (tok.long(), tok.float(), tok[0], torch.zeros(2, 1025, dtype=torch.int32), torch.zeros(0, 4, dtype=torch.int32), tok.numpy(), None):
        with pytest.raises(ValueError):
            pkg.event_attributes(bad, ops=ops)
    r, st = torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.int32)
    vals = np.arange(8.0)
    for args in ((r, r, st, vals, "x", 1.0, 1.0), (r, r, st, vals, "r", 0.0, 1.0), (r, r, st, vals, "r", 1.0, float("nan")), (r, r, st, vals, "r", True, 1.0),
                 (r, r[:, :7], st, vals, "r", 1.0, 1.0), (r, r, st.float(), vals, "r", 1.0, 1.0), (r.double(), r, st, vals, "r", 1.0, 1.0),
                 (r, r, st, vals[:7], "r", 1.0, 1.0), (r[:, :1], r[:, :1], st[:, :1], vals[:1], "r", 1.0, 1.0), (r, r, st, np.full(8, np.inf), "r", 1.0, 1.0),
                 (torch.zeros(4097, 2), torch.zeros(4097, 2), torch.zeros(4097, 2, dtype=torch.int32), vals[:2], "n", 1.0, 1.0)):
        with pytest.raises(ValueError):
            pkg.sweep_scores(*args, ops=ops)
    m = make_model(64, 32, ops=ops)
    x, c = torch.zeros(2, 6, dtype=torch.long), torch.zeros(2, 24)
    for kw in (dict(which="both"), dict(n_values=1), dict(n_values=65), dict(min_val=float("nan")), dict(max_val="1"), dict(r_std=0), dict(n_std=-1.0),
               dict(eos=400), dict(eps=(torch.zeros(2, 32), torch.zeros(2, 32)))):
        args = dict(which="r", min_val=-1.0, max_val=1.0, r_std=1.0, n_std=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            pkg.controllability(m, x, c, steps=5, **args)
    assert ops.calls == []
    # and a good call of each goes through
    at = pkg.event_attributes(tok.view(1, 3, 10), ops=ops, want_cells=True)
    assert at.status.shape == (1, 3) and at.rhythm.shape == (1, 3, ha.cells_ld_for(10, ha.DEFAULT)) and bool((at.status == ha.EMPTY).all())
    assert pkg.sweep_scores(r, r, st, vals, "r", 1.0, 1.0, ops=ops)["n_used"] == 4
    assert ops.calls == ["event_attributes", "sweep_scores"]


def _sampled_round(pkg, m, which, **kw):
    rs = np.random.RandomState(11)
    x, c = torch.from_numpy(rs.randint(0, 342, (5, 20))), torch.from_numpy(rs.rand(5, 24).astype(np.float32))
    g = torch.Generator().manual_seed(5)
    eps = (torch.randn(5, 8, 32, generator=g), torch.randn(5, 8, 32, generator=g))
    return x, c, eps, pkg.controllability(m, x, c, which, -2.0, 1.5, 0.19, 1.4, steps=40, eps=eps, **kw)


def test_controllability_on_stand_ins_is_sweep_then_attributes_then_scores():
    pkg = load_package()
    m = make_model(64, 32, ops=ha.attr_fake_ops())
    for which in ("r", "n"):
        x, c, eps, res = _sampled_round(pkg, m, which, sample=dict(temperature=1.0, seed=3))
        assert np.array_equal(res["values"], np.array([-2.0 + k * 3.5 / 8 for k in range(8)])) and res["values"].max() < 1.5
        tok, _ = pkg.fader_sweep(m, x, c, res["values"].astype(np.float32), steps=40, which=which, eps=eps, sample=dict(temperature=1.0, seed=3))
        assert torch.equal(tok, res["tokens"]) and tok.shape == (5, 8, 40)
        ref = ha.event_attributes_ref(tok.reshape(40, 40).numpy(), 40, ha.DEFAULT, ha.cells_ld_for(40, ha.DEFAULT))
        got = {k: res[k].reshape(-1).numpy() for k in ("r_density", "n_density", "status")}
        assert all(np.array_equal(got[k], ref[k]) for k in got)
        sc = ha.sweep_scores_ref(ref["r_density"].reshape(5, 8), ref["n_density"].reshape(5, 8), ref["status"].reshape(5, 8), res["values"],
                                 0 if which == "r" else 1, 0.19, 1.4)
        ha.same_scores(res, sc, 0.0, which)
        assert res["n_used"] >= 1 and np.isfinite([res[k] for k in ha.SCORE_KEYS]).all()          # a sampled decode of 40 tokens sounds notes


def test_evaluate_on_stand_ins_prints_the_reference_lines(capsys):
    pkg = load_package()
    m = make_model(64, 32, ops=ha.attr_fake_ops())

    class DS:
        def __len__(self):
            return 7

        def __getitem__(self, i):
            rs = np.random.RandomState(i)
            return rs.randint(0, 342, 20).astype(np.float32), None, None, rs.rand(24).astype(np.float32), 0.1, 1.0

    ev = pkg.GMMNoteEvaluator(DS(), epochs=2, num_of_samples=4)
    assert isinstance(ev, pkg.GMMRhythmEvaluator) and ev.which == "n"
    res = ev.evaluate(m, -1.0, 1.0, 0.2, 1.3, steps=30, sample=dict(temperature=1.0, seed=1))
    assert len(res) == 3 and all(isinstance(a, np.ndarray) and a.shape == (2,) for a in res)
    lines = [l for l in capsys.readouterr().out.split("\n") if l and not l.startswith("Samples used")]
    num = r"(-?\d[\d.e+-]*|nan)"
    pats = [r"Generator consistency:  " + num, r"Generator restrictiveness:  " + num, r"Generator monotonicity: " + num] * 2 + [
        "=" * 44, r"Consistency: %s \+/- %s" % (num, num), r"Restrictiveness: %s \+/- %s" % (num, num), r"Monotonicity: %s \+/- %s" % (num, num), "=" * 44]
    assert len(lines) == len(pats) and all(re.fullmatch(p, l) for p, l in zip(pats, lines)), lines
    assert float(re.fullmatch(pats[0], lines[0]).group(1)) == res[0][0]
