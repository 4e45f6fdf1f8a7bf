"""Event tokens <-> timed notes (notes.py, fn_notes_from_tokens / fn_tokens_from_notes), CPU side: the two statements of each direction against each
other and against the tokens -> notes step the attribute goldens pinned (helpers_attributes.tokens_to_notes), both round trips, a hand case per clause of
the definition, the host twin in a stand-alone sanitizer build, the answers of the entry points to bad arguments, and every ValueError of the Python
layer in front of stand-in ops."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_attributes as ha
import helpers_notes as hn
from mfn_import import ROOT, load_package

P = hn.DEFAULT
ON, OFF, SH = (lambda q: P["on_lo"] + q), (lambda q: P["off_lo"] + q), (lambda k: P["shift_lo"] + k - 1)
VEL = lambda v: P["vel_lo"] + (v - 1) // 2          # the token of velocity v: 64 bins of 2
EOS = P["eos"]


def _round_trip_rows():
    """(name, FnNoteParams dict, row): the fixture rows of helpers_attributes and its hand rows - 60 rows"""
    for g, p, names, tok in ha.fixture_streams():
        for name, row in zip(names, tok):
            yield g + " " + name, hn.from_attr_params(p), row
    for name, row in ha.hand_rows().items():
        yield "hand " + name, hn.DEFAULT, np.array(row, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the restatement
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_two_statements_of_tokens_to_notes_agree():
    seen = dict(ok=0, empty=0, overflow=0)
    for c in hn.token_cases():
        a = hn.notes_from_tokens_ref(c["tok"], c["steps"], c["p"], c["notes_ld"], hn.notes_of)
        b = hn.notes_from_tokens_ref(c["tok"], c["steps"], c["p"], c["notes_ld"], hn.notes_of_np)
        hn.same(a, b, hn.NOTE_KEYS, c["tag"])
        for k, v in (("ok", 0), ("empty", hn.EMPTY), ("overflow", hn.OVERFLOW)):
            seen[k] += int((a["status"] == v).sum())
        if c["notes_ld"] == c["steps"]:
            assert not (a["status"] == hn.OVERFLOW).any(), c["tag"]          # every note has its own note-on token
        if c["tag"] == "wide":
            assert len(set(a["notes"][..., 3].ravel().tolist())) > 10 and a["notes"][..., 2].max() > 64
        if c["tag"].startswith("n_vel 0"):
            assert set(a["notes"][..., 3].ravel().tolist()) == {0, 127}      # default_vel 500 counts as 127; 0 in the zeroed tails
    assert all(v > 0 for v in seen.values()), seen


def test_the_two_statements_of_notes_to_tokens_agree():
    seen = dict(ok=0, empty=0, overflow=0)
    for c in hn.span_cases():
        a = hn.tokens_from_notes_ref(c["notes"], c["spans"], c["steps"], c["p"], hn.tokens_of)
        b = hn.tokens_from_notes_ref(c["notes"], c["spans"], c["steps"], c["p"], hn.tokens_of_np)
        hn.same(a, b, hn.TOKEN_KEYS, c["tag"])
        for k, v in (("ok", 0), ("empty", hn.EMPTY), ("overflow", hn.OVERFLOW)):
            seen[k] += int((a["status"] == v).sum())
        assert a["n_tokens"].max() <= hn.MAX_TICK + 3 * 1024 + 1
        if c["tag"].startswith("n_shift 1:"):
            assert a["n_tokens"].max() > 100000                             # the true length, far behind `steps`
    assert all(v > 0 for v in seen.values()), seen


def test_statement_1_gives_the_notes_the_attribute_goldens_pinned():
    n = 0
    for name, p, row in _round_trip_rows():
        got = {(q, t0, t1) for t0, t1, q, _ in hn.notes_of(row, p)["kept"]}
        want = ha.tokens_to_notes(row, hn.to_attr_params(p))
        assert got == set(want) and len(got) == len(want), name
        n += 1
    assert n == 60


def test_notes_survive_tokens_and_attributes_survive_notes():
    """notes_of(tokens_of(N)) == N with velocities snapped; attributes_sets(tokens_of(notes_of(row))) == attributes_sets(row); steps 256 and status 0 on
    every row, so that truncation cannot hide a difference"""
    longest, ratio = 0, 0.0
    for name, p, row in _round_trip_rows():
        first = hn.notes_of(row, p)
        N = np.array(first["kept"], dtype=np.int32).reshape(-1, 4)
        span = (0, len(N), 0, max(first["t_end"], 1))
        for statement in (hn.tokens_of, hn.tokens_of_np):
            tk = statement(N, span, p, 256)
            assert tk["status"] == (0 if len(N) else hn.EMPTY) and tk["n_kept"] == len(N), name
            back = hn.notes_of(tk["tokens"], p)
            assert back["kept"] == hn.snapped(first["kept"], p), name
        longest = max(longest, tk["n_tokens"])
        used = int(np.flatnonzero(np.r_[row, EOS] == EOS)[0]) if p["eos"] >= 0 else len(row)
        if len(N):
            ratio = max(ratio, tk["n_tokens"] / max(used, 1))
        a, b = ha.attributes_sets(row, hn.to_attr_params(p)), ha.attributes_sets(tk["tokens"], hn.to_attr_params(p))
        for k in ("n_cells", "status", "c_r", "c_n"):
            assert a[k] == b[k], (name, k)
        assert np.array_equal(a["rhythm"], b["rhythm"]) and np.array_equal(a["notes"], b["notes"]), name
    print("longest re-tokenised row %d tokens, worst length ratio %.2f" % (longest, ratio))
    assert longest <= 256


# ------------------------------------------------------------------------------------------------------------------------------
# 2. hand cases, one per clause
# ------------------------------------------------------------------------------------------------------------------------------
def _tok(notes, span=None, steps=32, **kw):
    notes = np.array(notes, dtype=np.int32).reshape(-1, 4)
    span = (0, len(notes), 0, 1 << 20) if span is None else span
    p = dict(P, **kw)
    a, b = hn.tokens_of(notes, span, p, steps), hn.tokens_of_np(notes, span, p, steps)
    assert all(np.array_equal(a[k], b[k]) for k in hn.TOKEN_KEYS)
    return a


def _stream(res):
    return res["tokens"][:min(res["n_tokens"], len(res["tokens"]))].tolist()


def test_gaps_of_n_shift_n_shift_plus_1_and_twice_n_shift():
    assert _stream(_tok([(0, 100, 5, 100)])) == [VEL(100), ON(5), SH(100), OFF(5), EOS]
    assert _stream(_tok([(0, 101, 5, 100)])) == [VEL(100), ON(5), SH(100), SH(1), OFF(5), EOS]
    assert _stream(_tok([(0, 200, 5, 100)])) == [VEL(100), ON(5), SH(100), SH(100), OFF(5), EOS]
    assert _stream(_tok([(250, 251, 5, 100)])) == [SH(100), SH(100), SH(50), VEL(100), ON(5), SH(1), OFF(5), EOS]


def test_off_goes_before_on_at_one_tick_and_both_notes_survive():
    notes = [(0, 50, 7, 100), (50, 80, 7, 100)]
    res = _tok(notes)
    assert _stream(res) == [VEL(100), ON(7), SH(50), OFF(7), ON(7), SH(30), OFF(7), EOS]
    assert hn.notes_of(res["tokens"], P)["kept"] == [(0, 50, 7, 99), (50, 80, 7, 99)]          # 100 snaps to bin 49 = 99


def test_overlapping_notes_of_one_pitch_are_cut_by_the_re_strike_rule():
    res = _tok([(0, 50, 7, 100), (30, 80, 7, 100)])
    assert _stream(res) == [VEL(100), ON(7), SH(30), ON(7), SH(20), OFF(7), SH(30), OFF(7), EOS] and res["n_kept"] == 2
    # the earlier note ends at the later one's start, the later one at the first note-off that follows; the second note-off is ignored
    assert hn.notes_of(res["tokens"], P)["kept"] == [(0, 30, 7, 99), (30, 50, 7, 99)]


def test_a_velocity_token_only_where_the_bin_changes():
    res = _tok([(0, 10, 1, 64), (0, 10, 2, 63), (10, 20, 3, 65), (10, 20, 4, 66)])          # 63, 64 share bin 31; 65, 66 bin 32
    assert _stream(res) == [VEL(63), ON(1), ON(2), SH(10), OFF(1), OFF(2), VEL(65), ON(3), ON(4), SH(10), OFF(3), OFF(4), EOS]
    assert [n[3] for n in hn.notes_of(res["tokens"], P)["kept"]] == [63, 63, 65, 65]


def test_n_vel_0_neither_reads_nor_writes_velocity():
    res = _tok([(0, 10, 1, 64), (10, 20, 3, 20)], n_vel=0)
    assert _stream(res) == [ON(1), SH(10), OFF(1), ON(3), SH(10), OFF(3), EOS]
    row = [VEL(30), ON(1), SH(10), OFF(1)]
    assert hn.notes_of(row, dict(P, n_vel=0))["kept"] == [(0, 10, 1, 100)] and hn.notes_of(row, P)["kept"] == [(0, 10, 1, 29)]


def test_the_window_is_half_open_and_cuts_a_note_that_leaves_it():
    notes = [(100, 120, 1, 80), (200, 230, 2, 80), (180, 260, 3, 80), (99, 150, 4, 80)]
    res = _tok(notes, span=(0, 4, 100, 200))
    # the note starting at t_hi and the one starting before t_lo are dropped; the note ending behind t_hi is cut at it; times are relative to t_lo
    assert res["n_kept"] == 2 and _stream(res) == [VEL(80), ON(1), SH(20), OFF(1), SH(60), ON(3), SH(20), OFF(3), EOS]


def test_a_bad_pitch_is_dropped_and_velocities_are_clamped():
    res = _tok([(0, 10, -1, 80), (0, 10, 88, 80), (0, 10, 87, 0), (10, 20, 0, 200)])
    assert res["n_kept"] == 2 and _stream(res) == [VEL(1), ON(87), SH(10), OFF(87), VEL(127), ON(0), SH(10), OFF(0), EOS]


def test_unsorted_and_duplicated_input():
    a = _tok([(10, 20, 5, 80), (0, 10, 9, 80), (0, 10, 3, 80)])
    assert _stream(a) == [VEL(80), ON(3), ON(9), SH(10), OFF(3), OFF(9), ON(5), SH(10), OFF(5), EOS]
    d = _tok([(0, 10, 3, 80), (0, 10, 3, 80)])
    assert d["n_kept"] == 2 and _stream(d) == [VEL(80), ON(3), ON(3), SH(10), OFF(3), OFF(3), EOS]
    assert hn.notes_of(d["tokens"], P)["kept"] == [(0, 10, 3, 79)]           # the first of the two is re-struck at its own start and dropped


def test_a_row_that_just_fits_one_that_does_not_and_eos_on_the_last_column():
    notes = [(0, 10, 3, 80)]                                                  # VEL ON SH OFF EOS: 5 tokens
    fits, tight, over = _tok(notes, steps=6), _tok(notes, steps=5), _tok(notes, steps=4)
    assert (fits["n_tokens"], fits["status"], fits["tokens"].tolist()) == (5, 0, [VEL(80), ON(3), SH(10), OFF(3), EOS, P["pad"]])
    assert (tight["n_tokens"], tight["status"], tight["tokens"][-1]) == (5, 0, EOS)
    assert (over["n_tokens"], over["status"], over["tokens"].tolist()) == (5, hn.OVERFLOW, [VEL(80), ON(3), SH(10), OFF(3)])
    assert _tok(notes, steps=4, add_eos=0)["status"] == 0 and _tok(notes, steps=4, eos=-1)["n_tokens"] == 4


def test_a_span_is_cut_to_the_array_and_count_0_is_empty():
    notes = [(0, 10, 3, 80), (10, 20, 4, 80)]
    res = _tok(notes, span=(1, 5, 0, 100))
    assert res["n_kept"] == 1 and _stream(res) == [SH(10), VEL(80), ON(4), SH(10), OFF(4), EOS]
    assert _tok(notes, span=(-1, 2, 0, 100))["n_kept"] == 1
    for span in ((0, 0, 0, 100), (0, -4, 0, 100), (5, 3, 0, 100)):
        e = _tok(notes, span=span, steps=3)
        assert (e["n_kept"], e["n_tokens"], e["status"], e["tokens"].tolist()) == (0, 1, hn.EMPTY, [EOS, P["pad"], P["pad"]])
    big = np.array([(i, i + 1, 3, 80) for i in range(600)], dtype=np.int32)
    assert _tok(big, span=(0, 600, 0, 1000), steps=8)["n_kept"] == hn.NOTES_MAX


def test_the_velocity_bins():
    p = hn.clamped(P)
    assert p["vstep"] == 2 and [hn.bin_of_vel(v, p) for v in (1, 2, 3, 126, 127)] == [0, 0, 1, 62, 63]
    assert [hn.vel_of_bin(k, p) for k in (0, 1, 62, 63)] == [1, 3, 125, 127]
    for n_vel in (1, 32, 42, 64, 127, 128):
        q = hn.clamped(dict(P, n_vel=n_vel))
        assert all(hn.bin_of_vel(hn.vel_of_bin(k, q), q) == k for k in range(n_vel) if k * q["vstep"] < 127)
        assert all(0 <= hn.bin_of_vel(v, q) < n_vel for v in range(1, 128))


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
    src = os.path.join(ROOT, "music-fader-nets_amd", "csrc", "host", "notes_check.cpp")
    exe = str(tmp_path / "notes_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror", src, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    for c in hn.token_cases():
        ref = hn.notes_from_tokens_ref(c["tok"], c["steps"], c["p"], c["notes_ld"])
        rows, tok_ld = c["tok"].shape
        raw = _run(exe, fin, fout, i32(0, rows, c["steps"], tok_ld, c["notes_ld"], 0, 0, 0) + hn.params_bytes(c["p"]).tobytes()
                   + np.ascontiguousarray(c["tok"]).tobytes())
        body = np.frombuffer(raw, np.int32)
        assert body[0] == 0 and len(body) == 1 + rows * (4 * c["notes_ld"] + 3), c["tag"]
        got = dict(notes=body[1:1 + rows * 4 * c["notes_ld"]].reshape(rows, c["notes_ld"], 4))
        got["n_notes"], got["t_end"], got["status"] = body[1 + rows * 4 * c["notes_ld"]:].reshape(3, rows)
        hn.same(got, ref, hn.NOTE_KEYS, c["tag"])
    for c in hn.span_cases():
        if c.get("unspecified"):
            ref = None
        else:
            ref = hn.tokens_from_notes_ref(c["notes"], c["spans"], c["steps"], c["p"])
        rows, tok_ld = len(c["spans"]), c["tok_ld"]
        raw = _run(exe, fin, fout, i32(1, rows, c["steps"], tok_ld, len(c["notes"]), 0, 0, 0) + hn.params_bytes(c["p"]).tobytes()
                   + c["notes"].tobytes() + c["spans"].tobytes())
        body = np.frombuffer(raw, np.int32)
        assert body[0] == 0 and len(body) == 1 + rows * (tok_ld + 3), c["tag"]
        tok = body[1:1 + rows * tok_ld].reshape(rows, tok_ld)
        assert (tok[:, c["steps"]:] == -9).all(), c["tag"]                  # nothing behind `steps`
        if ref is not None:
            got = dict(tokens=tok[:, :c["steps"]])
            got["n_tokens"], got["n_kept"], got["status"] = body[1 + rows * tok_ld:].reshape(3, rows)
            hn.same(got, ref, hn.TOKEN_KEYS, c["tag"])
    # what the twin answers to bad sizes
    for hd, want in (((0, 1, 0, 4, 4, 0, 0, 0), -2), ((0, 1, 5, 4, 4, 0, 0, 0), -2), ((0, 1, 4, 3, 4, 0, 0, 0), -2)):
        raw = _run(exe, fin, fout, i32(*hd) + hn.params_bytes(P).tobytes() + np.zeros(4, np.int32).tobytes())
        assert np.frombuffer(raw, np.int32).tolist() == [want], hd
    for hd, want in (((1, 1, 0, 4, 1, 0, 0, 0), -2), ((1, 1, 5, 4, 1, 0, 0, 0), -2), ((1, 1, 4, 4, -1, 0, 0, 0), -2)):
        raw = _run(exe, fin, fout, i32(*hd) + hn.params_bytes(P).tobytes() + np.zeros(4 * max(hd[4], 0) + 4, np.int32).tobytes())
        assert np.frombuffer(raw, np.int32).tolist() == [want], hd


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the ABI without a GPU
# ------------------------------------------------------------------------------------------------------------------------------
def test_note_entry_points_argument_errors_without_gpu():
    load_package()
    from music_fader_nets_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "fadernets.h")).read()
    assert C.sizeof(_lib.FnNoteParams) == 64 == hn.PARAMS_DTYPE.itemsize and C.sizeof(_lib.FnNote) == 16 == C.sizeof(_lib.FnNoteSpan)
    assert [f[0] for f in _lib.FnNoteParams._fields_][:-1] == list(hn.FIELDS) and lib.fn_version() == 6
    for name, text in (("FN_NOTES_MAX", "512"), ("FN_NOTES_MAX_TICK", "(1 << 22)"), ("FN_NOTES_EMPTY", "1"), ("FN_NOTES_OVERFLOW", "2")):
        assert re.search(r"^#define %s %s$" % (name, re.escape(text)), hdr, re.M) and eval(text) == getattr(_lib, name), name
    assert (_lib.FN_NOTES_MAX, _lib.FN_NOTES_MAX_TICK, _lib.FN_NOTES_EMPTY, _lib.FN_NOTES_OVERFLOW) == (hn.NOTES_MAX, hn.MAX_TICK, hn.EMPTY, hn.OVERFLOW)
    assert _lib.FN_NOTES_MAX_TICK == _lib.FN_ATTR_MAX_STEPS * 4096
    buf = (C.c_int32 * 4096)()
    b = C.cast(buf, C.c_void_p)
    ok = dict(tokens=b, tok_ld=8, rows=2, steps=8, params=b, notes=b, notes_ld=8, n_notes=b, t_end=b, status=b)
    order = ("tokens", "tok_ld", "rows", "steps", "params", "notes", "notes_ld", "n_notes", "t_end", "status")
    call = lambda **kw: lib.fn_notes_from_tokens(*[dict(ok, **kw)[k] for k in order], None)
    for k in ("tokens", "params", "notes", "n_notes", "t_end", "status"):
        assert call(**{k: None}) == -1, k
    for kw in (dict(rows=0), dict(rows=-1), dict(steps=0), dict(steps=1025, tok_ld=1025), dict(tok_ld=7), dict(notes_ld=0), dict(notes_ld=-1)):
        assert call(**kw) == -2, kw
    assert call(tokens=None, rows=0) == -1                                     # null pointers are answered first
    ok = dict(notes=b, n_total=4, spans=b, rows=2, params=b, tokens=b, tok_ld=8, steps=8, n_tokens=b, n_kept=b, status=b)
    order = ("notes", "n_total", "spans", "rows", "params", "tokens", "tok_ld", "steps", "n_tokens", "n_kept", "status")
    call = lambda **kw: lib.fn_tokens_from_notes(*[dict(ok, **kw)[k] for k in order], None)
    for k in ("notes", "spans", "params", "tokens", "n_tokens", "n_kept", "status"):
        assert call(**{k: None}) == -1, k
    for kw in (dict(rows=0), dict(rows=-1), dict(steps=0), dict(steps=1025, tok_ld=1025), dict(tok_ld=7), dict(n_total=-1), dict(notes=None, n_total=-1)):
        assert call(**kw) == -2, kw
    assert call(spans=None, rows=0) == -1


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the Python layer: every ValueError before a launch; the two calls on stand-ins
# ------------------------------------------------------------------------------------------------------------------------------
def test_python_value_errors_come_before_any_launch():
    pkg = load_package()
    ops = hn.notes_fake_ops()
    NV = pkg.NoteVocab
    assert NV() == (2, 90, 88, 178, 100, 278, 64, 21)
    tok = torch.zeros(3, 10, dtype=torch.int32)
    bad_vocab = (None, (2, 90, 88), NV(n_pitch=0), NV(n_pitch=129), NV(off_lo=80), NV(on_lo=300), NV(n_pitch=89), NV(n_shift=0), NV(shift_lo=100),
                 NV(n_shift=101), NV(n_vel=65), NV(n_vel=129), NV(vel_lo=200), NV(n_vel=-1), NV(midi_lo=41), NV(midi_lo=-1), NV(n_vel=2.0), NV(on_lo=True))
    for kw in [dict(vocab=v) for v in bad_vocab] + [dict(eos=-1), dict(eos=342), dict(eos=1.0), dict(eos=True), dict(eos=5), dict(eos=200), dict(eos=300),
                                                    dict(default_vel=0), dict(default_vel=128), dict(default_vel=64.0)]:
        with pytest.raises(ValueError):
            pkg.tokens_to_notes(tok, ops=ops, **kw)
    for bad in (tok.long(), tok.float(), tok[0], torch.zeros(2, 1025, dtype=torch.int32), torch.zeros(0, 4, dtype=torch.int32), tok.numpy(), None):
        with pytest.raises(ValueError):
            pkg.tokens_to_notes(bad, ops=ops)
    notes, n = torch.zeros(3, 8, 4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    flat, spans = torch.zeros(9, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)
    for args, kw in (((notes,), {}), ((notes,), dict(n_notes=n[:2])), ((notes,), dict(n_notes=n.long())), ((notes, spans), dict(n_notes=n)),
                     ((torch.zeros(3, 513, 4, dtype=torch.int32),), dict(n_notes=n)), ((torch.zeros(3, 0, 4, dtype=torch.int32),), dict(n_notes=n)),
                     ((notes.long(),), dict(n_notes=n)), ((torch.zeros(3, 8, 3, dtype=torch.int32),), dict(n_notes=n)), ((notes.numpy(),), dict(n_notes=n)),
                     ((flat,), {}), ((flat, spans), dict(n_notes=n)), ((flat, spans.long()), {}), ((flat, spans[:, :3]), {}), ((flat, spans[:0]), {}),
                     ((flat, spans), dict(steps=0)), ((flat, spans), dict(steps=1025)), ((flat, spans), dict(steps=10.0)), ((flat, spans), dict(pad=-1)),
                     ((flat, spans), dict(pad=342)), ((flat, spans), dict(add_eos=1)), ((flat, spans), dict(eos=None)), ((flat, spans), dict(eos=100)),
                     ((flat, spans), dict(vocab=NV(n_vel=65)))):
        with pytest.raises(ValueError):
            pkg.notes_to_tokens(*args, ops=ops, **kw)
    for kw in (dict(names=["a.mid"]), dict(names=["a.mid", "", "c.mid"]), dict(qpm=97), dict(eos=5), dict(tokens=tok.long())):
        with pytest.raises(ValueError):
            pkg.write_midis("unused", **dict(dict(tokens=tok, ops=ops), **kw))
    assert ops.calls == [] and not os.path.exists("unused")
    # and a good call of each goes through
    res = pkg.tokens_to_notes(tok.view(1, 3, 10), ops=ops)
    assert res.notes.shape == (1, 3, 10, 4) and res.status.shape == (1, 3) and bool((res.status == hn.EMPTY).all())
    out = pkg.notes_to_tokens(flat, spans, add_eos=False, eos=None, steps=7, ops=ops)
    assert out[0].shape == (2, 7) and out[0].dtype == torch.int32 and out[1].tolist() == [0, 0]
    assert ops.calls == ["notes_from_tokens", "tokens_from_notes"]


def test_notes_feed_the_tokeniser_directly_and_files_hold_them(tmp_path):
    """tokens_to_notes -> notes_to_tokens(notes, n_notes=...) on stand-ins: the round trip of the fixture rows through the public calls; write_midis makes
    one decode call and its files read back as the notes"""
    pkg = load_package()
    ops = hn.notes_fake_ops()
    g, p, names, tok = ha.fixture_streams()[0]
    tok = torch.from_numpy(tok)
    res = pkg.tokens_to_notes(tok, ops=ops)
    back, n_tokens, n_kept, status = pkg.notes_to_tokens(res.notes, n_notes=res.n_notes, steps=256, ops=ops)
    assert torch.equal(n_kept, res.n_notes) and torch.equal(status, res.status) and int(n_tokens.max()) <= 256
    again = pkg.tokens_to_notes(back, ops=ops)
    for i in range(len(tok)):
        n = int(res.n_notes[i])
        assert [tuple(x) for x in again.notes[i, :n].tolist()] == hn.snapped([tuple(x) for x in res.notes[i, :n].tolist()], hn.DEFAULT), names[i]
    ops.calls.clear()
    paths = pkg.write_midis(str(tmp_path / "out"), tok.view(3, 11, 100), ops=ops)
    assert ops.calls == ["notes_from_tokens"] and len(paths) == 33 and paths[12].endswith("001_01.mid")
    for i, path in enumerate(paths):
        n = int(res.n_notes[i])
        assert torch.equal(pkg.read_midi(path).notes, res.notes[i, :n]), names[i]
    f = tmp_path / "row.mid"
    pkg.write_midi(str(f), tok[20], ops=ops)                                  # a token row is decoded first
    assert torch.equal(pkg.read_midi(str(f)).notes, res.notes[20, :int(res.n_notes[20])])
