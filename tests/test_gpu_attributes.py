"""Controllability metrics on a real MI355X: fn_event_attributes bit for bit against the restatement on every case the CPU tests run through the two
statements and the host twin (per-cell outputs requested and not, sentinel columns and sentinel bytes), fn_sweep_scores against the restatement, and
controllability / evaluate end to end at hidden 64: the densities of the tokens the same fader_sweep call returns, a second call with the same bits,
greedy, sampled and constrained decodes - and under max_polyphony = 2 no cell with more than two notes."""
import re

import numpy as np
import pytest
import torch

import helpers_attributes as ha
from helpers import make_model
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ha.kernel_cases()
TAIL = 64


def _ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(DEV)


@pytest.mark.parametrize("case", CASES, ids=[c["tag"].replace(" ", "_") for c in CASES])
def test_event_attributes_kernel(case):
    """tokens as a view of a wider matrix whose last columns are sentinels (a note-on: reading one changes the result), outputs that start as
    sentinels, per-cell outputs in front of sentinel bytes; then the same call without the per-cell outputs"""
    ops = _ops()
    rows, steps, cells_ld = case["tok"].shape[0], case["steps"], case["cells_ld"]
    ref = ha.event_attributes_ref(case["tok"], steps, case["p"], cells_ld)
    tok = torch.from_numpy(case["tok"]).to(DEV)
    prm = torch.from_numpy(ha.params_bytes(case["p"])).to(DEV)

    def outputs():
        i32, f32 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.float32, device=DEV)
        return dict(n_cells=torch.full((rows,), -9, **i32), status=torch.full((rows,), -9, **i32), r_density=torch.full((rows,), -9.0, **f32),
                    n_density=torch.full((rows,), -9.0, **f32), c_r=torch.full((rows,), -9, **i32), c_n=torch.full((rows,), -9, **i32))

    out = outputs()
    bufs = [torch.full((rows * cells_ld + TAIL,), ha.SENTINEL_CELL, dtype=torch.uint8, device=DEV) for _ in range(2)]
    cells = [b[:rows * cells_ld].view(rows, cells_ld) for b in bufs]
    ops.event_attributes(tok[:, :steps], steps, prm, rhythm=cells[0], notes=cells[1], cells_ld=cells_ld, **out)
    out2 = outputs()
    ops.event_attributes(tok[:, :steps], steps, prm, cells_ld=cells_ld, **out2)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["rhythm"], got["notes"] = cells[0].cpu().numpy(), cells[1].cpu().numpy()
    ha.same_attributes(got, ref, case["tag"])
    ha.same_attributes({k: v.cpu().numpy() for k, v in out2.items()}, ref, case["tag"] + " without cells", cells=False)
    assert all(bool((b[rows * cells_ld:] == ha.SENTINEL_CELL).all()) for b in bufs)
    assert torch.equal(tok.cpu(), torch.from_numpy(case["tok"]))


def _device_scores(ops, args):
    r, n, status, values, which, r_std, n_std = args
    scores, n_used = torch.full((4,), -9.0, dtype=torch.float64, device=DEV), torch.full((1,), -9, dtype=torch.int32, device=DEV)
    ops.sweep_scores(torch.from_numpy(r).to(DEV), torch.from_numpy(n).to(DEV), torch.from_numpy(status).to(DEV), torch.from_numpy(values).to(DEV), which,
                     r_std, n_std, scores, n_used)
    return dict(zip(ha.SCORE_KEYS, scores.cpu().tolist()), n_used=int(n_used.item()))


def test_sweep_scores_kernel():
    """the fixture's cases (S 1 / 5 / 67, flat, linear and decreasing rows, invalid entries, nothing used) and shapes at the caps' ends: 64 values,
    two values, more samples than one pass of the 16 wavefronts; within 1e-10, n_used exact, NaN where nothing is used; a second launch gives the
    same bits"""
    ops = _ops()
    cases = [(c[0], c[1:]) for c in ha.score_cases() + [ha.unused_scores_case()]]
    rs = np.random.RandomState(3)
    for S, Vn in ((1000, 64), (17, 2), (33, 63)):
        r, n = rs.rand(S, Vn).astype(np.float32), (4 * rs.rand(S, Vn)).astype(np.float32)
        status = (rs.rand(S, Vn) < 0.02 / Vn * 8).astype(np.int32) * ha.EMPTY
        r[1] = 0.5
        cases.append(("S%d Vn%d" % (S, Vn), (r, n, status, np.sort(rs.randn(Vn)), S % 2, 0.21, 1.1)))
    for tag, args in cases:
        got, ref = _device_scores(ops, args), ha.sweep_scores_ref(*args)
        ha.same_scores(got, ref, 1e-10, tag)
        again = _device_scores(ops, args)
        assert all(np.float64(got[k]).tobytes() == np.float64(again[k]).tobytes() for k in ha.SCORE_KEYS), tag
    assert np.isnan(_device_scores(ops, cases[len(ha.score_cases())][1])["monotonicity"])


def _inputs():
    rs = np.random.RandomState(11)
    x, c = torch.from_numpy(rs.randint(0, 342, (5, 20))).to(DEV), torch.from_numpy(rs.rand(5, 24).astype(np.float32)).to(DEV)
    g = torch.Generator().manual_seed(5)
    return x, c, (torch.randn(5, 8, 32, generator=g), torch.randn(5, 8, 32, generator=g))


@pytest.mark.parametrize("mode", ["greedy", "sample", "constrained"])
def test_controllability_end_to_end(mode):
    """5 samples x 8 values x 100 steps at hidden 64: the result is the restatement applied to the tokens the same fader_sweep call returns with the
    same eps; a second call gives the same bits; with Constraints(max_polyphony=2, no_reonset, off_needs_on) no cell holds more than two notes"""
    pkg = load_package()
    m = make_model(64, 32, device=DEV)
    x, c, eps = _inputs()
    con = pkg.Constraints(max_polyphony=2, no_reonset=True, off_needs_on=True)
    kw = dict(greedy={}, sample=dict(sample=dict(temperature=1.0, seed=3)), constrained=dict(sample=dict(temperature=1.0, seed=3), constraints=con))[mode]
    which = "n" if mode == "sample" else "r"
    res = pkg.controllability(m, x, c, which, -2.0, 1.5, 0.19, 1.4, steps=100, eps=eps, **kw)
    assert np.array_equal(res["values"], np.array([-2.0 + k * 3.5 / 8 for k in range(8)]))
    tok, _ = pkg.fader_sweep(m, x, c, res["values"].astype(np.float32), steps=100, which=which, eps=eps, **kw)
    assert tok.shape == (5, 8, 100) and torch.equal(tok, res["tokens"])
    ref = ha.event_attributes_ref(tok.reshape(40, 100).cpu().numpy(), 100, ha.DEFAULT, ha.cells_ld_for(100, ha.DEFAULT))
    for k in ("r_density", "n_density", "status"):
        g = res[k].reshape(-1).cpu().numpy()
        assert res[k].is_cuda and g.dtype == ref[k].dtype and g.tobytes() == ref[k].tobytes(), (mode, k)
    sc = ha.sweep_scores_ref(ref["r_density"].reshape(5, 8), ref["n_density"].reshape(5, 8), ref["status"].reshape(5, 8), res["values"],
                             0 if which == "r" else 1, 0.19, 1.4)
    ha.same_scores(res, sc, 1e-10, mode)
    again = pkg.controllability(m, x, c, which, -2.0, 1.5, 0.19, 1.4, steps=100, eps=eps, **kw)
    assert torch.equal(again["tokens"], res["tokens"]) and again["n_used"] == res["n_used"]
    assert all(np.float64(again[k]).tobytes() == np.float64(res[k]).tobytes() for k in ha.SCORE_KEYS)
    assert all(torch.equal(again[k].view(torch.int32), res[k].view(torch.int32)) for k in ("r_density", "n_density", "status"))
    if mode != "greedy":
        assert res["n_used"] >= 1 and np.isfinite([res[k] for k in ha.SCORE_KEYS]).all()          # a sampled decode of 100 tokens sounds notes
    at = pkg.event_attributes(tok, want_cells=True)
    cells = ha.event_attributes_ref(tok.reshape(40, 100).cpu().numpy(), 100, ha.DEFAULT, at.notes.shape[-1])
    assert np.array_equal(at.notes.reshape(40, -1).cpu().numpy(), cells["notes"]) and np.array_equal(at.rhythm.reshape(40, -1).cpu().numpy(), cells["rhythm"])
    if mode == "constrained":
        assert int(at.notes.max()) <= 2 and int((at.status == 0).sum()) >= 20
    if mode == "sample":
        assert int(at.notes.max()) > 2                                       # the witness: unconstrained, the same sampler stacks more notes


def test_evaluate_prints_the_reference_lines(capsys):
    pkg = load_package()
    m = make_model(64, 32, device=DEV)

    class DS:
        def __len__(self):
            return 7

        def __getitem__(self, i):
            rs = np.random.RandomState(i)
            return rs.randint(0, 342, 20).astype(np.float32), None, None, rs.rand(24).astype(np.float32), 0.1, 1.0

    res = pkg.GMMRhythmEvaluator(DS(), epochs=2, num_of_samples=6).evaluate(m, -1.0, 1.0, 0.2, 1.3, sample=dict(temperature=1.0, seed=1))
    assert len(res) == 3 and all(isinstance(a, np.ndarray) and a.shape == (2,) and np.isfinite(a).all() for a in res)
    lines = [l for l in capsys.readouterr().out.split("\n") if l and not l.startswith("Samples used")]
    num = r"(-?\d[\d.e+-]*|nan)"
    pats = [r"Generator consistency:  " + num, r"Generator restrictiveness:  " + num, r"Generator monotonicity: " + num] * 2 + [
        "=" * 44, r"Consistency: %s \+/- %s" % (num, num), r"Restrictiveness: %s \+/- %s" % (num, num), r"Monotonicity: %s \+/- %s" % (num, num), "=" * 44]
    assert len(lines) == len(pats) and all(re.fullmatch(p, l) for p, l in zip(pats, lines)), lines
