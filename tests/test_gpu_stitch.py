"""Decoded windows back into pieces on a real MI355X: fn_notes_stitch exactly against statement 2 of tests/helpers_stitch.py on every case the CPU tests
run through the two statements and the host twin (guard rows behind out_ld, sentinel slots behind dec_n and behind dec_ld, untouched inputs), against the
host twin on a mixed case, and transfer_piece / transfer_midi / the script on the device against the restatement applied to the device's own tokens."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers_stitch as hs
from helpers import make_model
from mfn_import import ROOT, load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = hs.stitch_cases()
_id = lambda c: c["tag"].replace(" ", "_")
GUARD = 64          # note slots behind out[V][out_ld] that must come back untouched


def _ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(DEV)


def _stitch_on_device(ops, c):
    S, V, out_ld = c["S"], c["V"], c["out_ld"]
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("dec", "dec_n", "dec_end", "src", "spans", "mode")}
    buf = torch.full(((V * out_ld + GUARD) * 4,), -9, dtype=torch.int32, device=DEV)
    out = buf[:V * out_ld * 4].view(V, out_ld, 4)
    win_first = torch.full((V * (S + 1) + 8,), -9, dtype=torch.int32, device=DEV)
    out_n, status = (torch.full((V,), -9, dtype=torch.int32, device=DEV) for _ in range(2))
    ops.notes_stitch(t["dec"], c["dec_ld"], t["dec_n"], t["dec_end"], t["src"], t["spans"], t["mode"], out, win_first[:V * (S + 1)].view(V, S + 1), out_n, status)
    torch.cuda.synchronize()
    assert bool((buf[V * out_ld * 4:] == -9).all()) and bool((win_first[V * (S + 1):] == -9).all()), c["tag"]
    assert all(torch.equal(t[k].cpu(), torch.from_numpy(np.ascontiguousarray(c[k]))) for k in t), c["tag"]
    return dict(notes=out.cpu().numpy(), n_notes=out_n.cpu().numpy(), win_first=win_first[:V * (S + 1)].view(V, S + 1).cpu().numpy(), status=status.cpu().numpy())


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_notes_stitch_kernel(case):
    """dec is (S*V, rs, 4) with dec_ld <= rs slots in use and a sentinel note in every slot behind dec_n; out lies in front of guard slots and starts
    as sentinels: the notes, zeros up to out_ld, nothing behind it"""
    hs.same(_stitch_on_device(_ops(), case), hs.stitch_ref(case), case["tag"])


def test_kernel_equals_the_host_twin_on_a_mixed_case(tmp_path):
    """the twin as a plain stand-alone program (csrc/host/stitch_check.cpp), its answer against the device's, word for word"""
    c = next(c for c in CASES if c["tag"] == "S 65 V 3")
    assert {0, 1, 2, 7} <= set(c["mode"].tolist())
    exe = str(tmp_path / "stitch_check")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "music-fader-nets_amd", "csrc", "host", "stitch_check.cpp"), "-o", exe], check=True,
                   capture_output=True, timeout=300)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    S, V, out_ld = c["S"], c["V"], c["out_ld"]
    with open(fin, "wb") as f:
        f.write(np.array([S, V, c["dec"].shape[1], c["dec_ld"], len(c["src"]), out_ld, 0, 0], np.int32).tobytes())
        f.write(b"".join(np.ascontiguousarray(c[k]).tobytes() for k in ("dec", "dec_n", "dec_end", "src", "spans", "mode")))
    subprocess.run([exe, fin, fout], check=True, capture_output=True, timeout=60)
    body = np.fromfile(fout, np.int32)
    a, b = 1 + V * 4 * out_ld, 1 + V * 4 * out_ld + V * (S + 1)
    assert body[0] == 0 and len(body) == b + 2 * V
    twin = dict(notes=body[1:a].reshape(V, out_ld, 4), win_first=body[a:b].reshape(V, S + 1), n_notes=body[b:b + V], status=body[b + V:])
    hs.same(_stitch_on_device(_ops(), c), twin, c["tag"])


def _piece_kw():
    g = torch.Generator().manual_seed(5)
    return dict(eps=(torch.randn(6, 32, generator=g), torch.randn(6, 32, generator=g)), steps=40, sample=dict(temperature=1.0, seed=3))


def test_transfer_piece_on_the_device():
    """seeded model (hidden 64, Z 32), the hand piece, two amounts, both fits: the stitched pieces equal the restatement applied to the device's own
    tokens and `used`; a second call with another lmbda and curve on the same shapes gives that call's result - the settings are device data"""
    pkg = load_package()
    m = make_model(64, 32, device=DEV)
    midi = hs.hand_midi(pkg)
    seg = pkg.midi_segments(midi, device=DEV)
    spans, status = seg["spans"].cpu().numpy(), seg["status"].cpu().numpy()
    assert status.tolist() == [0, 0, 0, hs.EMPTY, hs.OVERFLOW, 0]
    for fit in ("clip", "scale"):
        res = pkg.transfer_piece(m, midi, lmbda=(1.0, -0.5), fit=fit, **_piece_kw())
        assert all(t.is_cuda for t in res) and res.tokens.shape == (6, 2, 40) and res.notes.shape == (2, len(midi.notes) + 7 * 40, 4)
        hs.check_transfer(pkg, midi, res, fit, spans, status)
        assert bool(res.used[[0, 1, 2, 5]].any()) and not bool(res.used[[3, 4]].any())          # a sampled decode of 40 tokens sounds notes
        again = pkg.transfer_piece(m, midi, lmbda=(-2.0, 0.25), curve=[1.0, 0.5, 0.0, 1.0, 2.0, -1.0], fit=fit, **_piece_kw())
        hs.check_transfer(pkg, midi, again, fit, spans, status)
        assert not torch.equal(again.tokens, res.tokens)
    greedy = pkg.transfer_piece(m, midi, lmbda=0.5, only_kept=True, steps=64)
    hs.check_transfer(pkg, midi, greedy, "clip", spans, status, ok=seg["keep"].cpu().numpy())


def test_transfer_midi_round_trip_on_the_device(tmp_path):
    pkg = load_package()
    m = make_model(64, 32, device=DEV)
    src = str(tmp_path / "in.mid")
    pkg.write_midi(src, hs.hand_midi(pkg).notes)
    midi = pkg.read_midi(src)
    res = pkg.transfer_piece(m, midi, lmbda=(1.0, -1.0), fit="scale", **_piece_kw())
    paths = pkg.transfer_midi(m, src, str(tmp_path / "out"), lmbda=(1.0, -1.0), fit="scale", **_piece_kw())
    assert len(paths) == 2
    for v, path in enumerate(paths):
        want = hs.tuples(res.notes[v].cpu(), res.n_notes[v])
        back = hs.tuples(pkg.read_midi(path).notes)
        assert hs.events(back) == hs.events(want) and len(back) == len(want) > len(midi.notes) // 2
        assert open(path, "rb").read() == pkg.midi.midi_bytes(np.array(want))


def test_the_script_turns_a_file_into_one_file_of_the_same_length(tmp_path):
    """python transfer_midi.py --config tests/golden/gmm_model_config.json in.mid out.mid --lmbda 1.0 on seeded initial weights: the output covers the
    input's length, and the windows that cannot be transferred (the empty one, the one that overflows 100 tokens) and the tail are the input's notes"""
    pkg = load_package()
    src, dst = str(tmp_path / "in.mid"), str(tmp_path / "out.mid")
    pkg.write_midi(src, hs.hand_midi(pkg).notes)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "transfer_midi.py"), "--config", os.path.join(ROOT, "tests", "golden", "gmm_model_config.json"), src,
                        dst, "--lmbda", "1.0", "--temperature", "1.0", "--seed", "3"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "seeded initial weights" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
    a, b = pkg.read_midi(src), pkg.read_midi(dst)
    got = set(hs.tuples(b.notes))
    assert all(n in got for n in hs.tuples(a.notes[19:64])) and all(n in got for n in hs.tuples(a.notes[-2:]))
    assert sum(1 for n in hs.tuples(b.notes) if 800 <= n[0] < 1000) == 45 and not any(600 <= n[0] < 800 for n in hs.tuples(b.notes))
    assert int(b.notes[:, 1].max()) >= 1230 and b.beats.numel() >= 25                # up to the tail's end
