#!/usr/bin/env python3
"""Golden fixture of the controllability metrics (include/fadernets.h, fn_event_attributes / fn_sweep_scores): ``attributes.npz``.

Runs ONLY in the build container.  The reference's own code is executed, not restated, taken by AST because its modules import the MIDI stack:
  * ``parse_pretty_midi`` (the vendored piano-roll fill), ``convert_pr_to_pitch_lst``, ``pitch_lst_to_rhythm`` from ``polyphonic_event_based_v2.py``;
  * ``get_classes``, ``BaseEvaluator``, ``RhythmEvaluator``, ``NoteEvaluator`` (the calculate_* methods) from ``test_class.py``, with scikit-learn's
    ``LinearRegression``;
  * the note density as ``get_music_attributes`` (ptb_v2.py:139-140) takes it: ``len`` of every cell's pitch list.
``parse_pretty_midi`` gets a stand-in for the PrettyMIDI object: no time-signature changes, ``estimate_beat_start() = 0``, beats at the multiples of
0.5 s up to and including floor(end / 0.5) * 0.5, one non-drum instrument whose notes (start t0 / 100, end t1 / 100, velocity 100) are listed in
closing order.  The step from tokens to those notes is OURS (tests/helpers_attributes.tokens_to_notes): Magenta's decoder is not at hand.

Arrays only.  Per group g of streams ("d": the default vocabulary, "w": 128 pitches): g/tokens, g/params (the ten FnAttrParams fields), g/names,
g/n_cells, g/r_density, g/n_density (float64 as the reference returns them), g/c_r, g/c_n, g/rhythm, g/notes (rows, max cells; 255 behind n_cells),
g/roll (all rows' cells x 128, bits packed) with g/roll_start.  Per score case k: s<k>/r, n, status, values, meta (which, r_std, n_std),
s<k>/scores (consistency, restrictiveness, monotonicity, variance as evaluate forms them) and s<k>/n_used.
"""
import ast
import os
import sys
from collections import Counter

import numpy as np
from sklearn.linear_model import LinearRegression

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import helpers_attributes as ha  # noqa: E402


def extract(path, names, ns):
    tree = ast.parse(open(os.path.join(REF, path)).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert {n.name for n in body} == set(names), (path, names)
    exec(compile(ast.Module(body=body, type_ignores=[]), path + "[extract]", "exec"), ns)


class Note:
    def __init__(self, pitch, start, end):
        self.pitch, self.start, self.end, self.velocity = pitch, start, end, 100


class Instrument:
    is_drum = False

    def __init__(self, notes):
        self.notes = notes


class StandInMidi:
    """what parse_pretty_midi asks of a PrettyMIDI object"""

    def __init__(self, notes):
        self.time_signature_changes = []
        self.instruments = [Instrument([Note(p, t0 / 100, t1 / 100) for p, t0, t1 in notes])]
        self.t_last = max(t1 for _, _, t1 in notes)

    def estimate_beat_start(self):
        return 0

    def get_tempo_changes(self):
        return np.array([0.0]), np.array([120.0])

    def get_beats(self, start_time=0.0):
        assert start_time == 0
        return np.arange(self.t_last // 50 + 1) * 0.5


def main():
    ns = dict(np=np, Counter=Counter, LinearRegression=LinearRegression)
    extract("polyphonic_event_based_v2.py", {"parse_pretty_midi", "convert_pr_to_pitch_lst", "pitch_lst_to_rhythm"}, ns)
    extract("test_class.py", {"get_classes", "BaseEvaluator", "RhythmEvaluator", "NoteEvaluator"}, ns)
    out = {}
    for g, p, names, tok in ha.fixture_streams():
        R = tok.shape[0]
        rec = dict(n_cells=np.zeros(R, np.int32), r_density=np.zeros(R), n_density=np.zeros(R), c_r=np.zeros(R, np.int32), c_n=np.zeros(R, np.int32))
        rolls, per_cell = [], []
        for i in range(R):
            notes = ha.tokens_to_notes(tok[i], p)
            assert all(t1 < 15000 for _, _, t1 in notes)
            assert not notes or max(t1 for _, _, t1 in notes) >= 50          # with one beat time the fill raises (:329)
            if not notes:                                   # `if len(track) < 1: continue`, test_class.py:134
                rolls.append(np.zeros((0, 128), bool)), per_cell.append(([], []))
                continue
            pr = ns["parse_pretty_midi"](StandInMidi(notes), beat_resolution=4)
            pitch_lst, _ = ns["convert_pr_to_pitch_lst"](pr)
            rhythm = ns["pitch_lst_to_rhythm"](pitch_lst)
            note = np.array([len(k) for k in pitch_lst])
            rd, nd, c_r, c_n = ns["get_classes"](rhythm, note)
            rec["n_cells"][i], rec["r_density"][i], rec["n_density"][i], rec["c_r"][i], rec["c_n"][i] = len(pr), rd, nd, c_r, c_n
            rolls.append(np.asarray(pr) > 0), per_cell.append((rhythm, list(note)))
        width = max(1, int(rec["n_cells"].max()))
        rhythm, notes = np.full((R, width), 255, np.uint8), np.full((R, width), 255, np.uint8)
        for i, (rh, nt) in enumerate(per_cell):
            rhythm[i, :len(rh)], notes[i, :len(nt)] = rh, nt
        P = g + "/"
        out[P + "tokens"], out[P + "params"], out[P + "names"] = tok, np.array([p[k] for k in ha.FIELDS], np.int32), np.array(names)
        for k, v in rec.items():
            out[P + k] = v
        out[P + "rhythm"], out[P + "notes"] = rhythm, notes
        out[P + "roll"] = np.packbits(np.concatenate(rolls, axis=0), axis=1)
        out[P + "roll_start"] = np.concatenate([[0], np.cumsum(rec["n_cells"])]).astype(np.int32)
        print(g, R, "rows, n_cells", rec["n_cells"].tolist())

    for k, (tag, r, n, status, values, which, r_std, n_std) in enumerate(ha.score_cases() + [ha.unused_scores_case()]):
        ev = (ns["RhythmEvaluator"] if which == 0 else ns["NoteEvaluator"])(None)
        used = [s for s in range(r.shape[0]) if not status[s].any()]
        P = "s%d/" % k
        out[P + "r"], out[P + "n"], out[P + "status"], out[P + "values"] = r, n, status, values
        out[P + "meta"], out[P + "tag"], out[P + "n_used"] = np.array([which, r_std, n_std]), np.array(tag), np.array(len(used), np.int32)
        if not used:
            out[P + "scores"] = np.full(4, np.nan)
            continue
        # test_class.py:141-175 for the samples that are kept
        r_all, n_all, result = [], [], []
        for s in used:
            r_new, n_new = [float(x) for x in r[s]], [float(x) for x in n[s]]
            r_all.append(np.array(r_new)), n_all.append(np.array(n_new))
            result.append(ev.calculate_monotonicity(r_new, n_new, values))
        r_all, n_all = np.array(r_all) / r_std, np.array(n_all) / n_std
        out[P + "scores"] = np.array([1 - ev.calculate_consistency(r_all, n_all), 1 - ev.calculate_restrictiveness(r_all, n_all),
                                      sum(result) / len(result), ev.calculate_variance(r_all, n_all)], np.float64)
        print(tag, out[P + "scores"])
    path = os.path.join(HERE, "attributes.npz")
    np.savez_compressed(path, **out)
    print("attributes ->", path, "%.1f KB" % (os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
