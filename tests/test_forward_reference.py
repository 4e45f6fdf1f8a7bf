"""The per-block check of the forward-only paths (helpers_forward.check_forward_outputs) on the CPU: tests/fake_ops.py stands in for the kernels under
the real Engine / model at every case and path test_gpu_forward.py runs.  Asserted here: the unmodified stand-in passes with ratio <= FORWARD_F / 2,
every input condition holds (the references assert them), FORWARD_F obeys its rule, planted faults - edits of CPU arrays - are rejected while the old
elementwise rtol = atol = 1e-4 accepts them (old_metric_accepts, stated per fault), and the launches of every forward-only call, planned by
fn_gru_fwd_plan at 256 compute units with gates = NULL, reach the kernels the GPU tests expect."""
import functools
import os

import numpy as np
import pytest

from fake_ops import FakeOps
from helpers_forward import (FORWARD_F, FORWARD_F_CAP, FORWARD_ONLY, FORWARD_PATHS, PATH_NAMES, check_forward_only_kernels, check_forward_outputs,
                             forward_line, forward_runs, make_launch_log, old_metric_accepts, planned_launches, run_forward_path)
from helpers_step import GMVAE_CASES, gmvae_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [(p, cid) for p, cid, _ in forward_runs(ariths=False)]
LaunchLog = make_launch_log(FakeOps)


@functools.lru_cache(maxsize=None)
def _run(path, cid):
    """(outputs, references, engine, launch log) of the stand-in on one path and case; run once per module"""
    ops = LaunchLog()
    got, ref, eng = run_forward_path(path, gmvae_case(cid), ops=ops)
    return got, ref, eng, ops.log


def _rejected(got, ref, names=None):
    """the checker's complaint about `got`, or None"""
    try:
        check_forward_outputs(got, ref, names=names)
    except AssertionError as e:
        return str(e)
    return None


def test_the_table_of_paths_covers_what_it_says():
    assert {c["id"] for c in GMVAE_CASES} == set(FORWARD_PATHS["engine"][0])                     # the engine path runs every case
    assert set(FORWARD_PATHS) == set(PATH_NAMES) == set(FORWARD_ONLY) | {"saved"}
    ariths = forward_runs()
    assert ("engine", "g", "bf16x6") in ariths and ("saved", "g", "bf16x6") in ariths and ("engine", "h", "bf16x6") in ariths
    assert len(set(ariths)) == len(ariths) and {(p, c) for p, c, _ in ariths} == set(RUNS)


@pytest.mark.parametrize("path,cid", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_stand_in_passes_per_block(path, cid):
    got, ref, _, _ = _run(path, cid)
    st = check_forward_outputs(got, ref, names=PATH_NAMES[path])       # ratio <= FORWARD_F, exact zeros, y = the float64 argmax (references: input conditions)
    assert st["worst"][0] <= FORWARD_F / 2, st["worst"]
    if "logits_pad" in got:
        assert st["zero_blocks"] > 0
    print()
    print(forward_line(path, cid, "f32", "fake-cpu", st))


def test_F_obeys_its_rule():
    """one power of two for every case, path and quantity, <= 32, at least twice the worst ratio of the stand-in"""
    worst = max((check_forward_outputs(_run(*r)[0], _run(*r)[1], names=PATH_NAMES[r[0]])["worst"][:2] + r for r in RUNS))
    assert FORWARD_F <= FORWARD_F_CAP == 32 and FORWARD_F & (FORWARD_F - 1) == 0
    assert worst[0] <= 16, "the stand-in alone exceeds 16: fix the inputs or the stand-in, not the cap (%s)" % (worst,)
    assert 2 * worst[0] <= FORWARD_F, worst


def test_profile_names_F_and_every_run():
    text = open(os.path.join(ROOT, "profiles", "forward_fp64_errors.txt")).read()
    assert "F = %d" % FORWARD_F in text.splitlines()[0]
    fake, gpu = text.split("# ---- MI355X")
    for path, cid in RUNS:
        assert any(l.split()[:2] == [path, cid] for l in fake.splitlines()), (path, cid)
    for path, cid, arith in forward_runs():
        assert any(l.split()[:3] == [path, cid, arith] for l in gpu.splitlines()), (path, cid, arith)


@pytest.mark.parametrize("path,cid", [r for r in RUNS if r[0] in FORWARD_ONLY], ids=["%s-%s" % r for r in RUNS if r[0] in FORWARD_ONLY])
def test_forward_only_launches_reach_the_expected_kernels(path, cid):
    """every gru_seq_fwd launch of the call carries gates = None; fn_gru_fwd_plan (256 compute units, made-up addresses) then names no ping-pong and no
    bf16 x 6 kernel, takes a weight-stationary gru_fwd_persist_kernel for case g's pipeline launches, the per-step kernel only where no
    weight-stationary candidate is listed in front of it or persist_dec is off - and refuses every one of these launches the bf16 x 6 arithmetic"""
    log = _run(path, cid)[3]
    assert log and all(s.get("gates") is None for scans, _ in log for s in scans)
    label = check_forward_only_kernels(planned_launches(log), gmvae_case(cid))
    assert all(not cands for _, _, _, cands, _, _ in planned_launches(log, x6=True))
    if cid == "g" and path in ("engine", "dropin"):
        assert "fwd_persist<4, 1, 2, 4>" in label and "fwd_persist<2, 2, 2, 4>" in label and "step" not in label, label
    if cid == "e" and path == "engine":
        assert "fwd_step" in label


def test_the_saved_path_keeps_its_gates():
    log = _run("saved", "g")[3]
    assert log and all(s.get("gates") is not None for scans, _ in log for s in scans)
    assert any(c[0].startswith("gru_fwd_pp_kernel") for _, _, _, c, _, _ in planned_launches(log))


# ---- planted faults: the new check rejects them, the elementwise rtol = atol = 1e-4 accepts them -------------------------------------------------------
def _clean(cid):
    got, ref, eng, _ = _run("engine", cid)
    assert _rejected(got, ref) is None and old_metric_accepts(got, ref)
    return {k: np.array(v.numpy() if hasattr(v, "numpy") else v) for k, v in got.items()}, ref, eng


def _into_tolerance(clean, faulty, size=5e-5):
    """clean + s (faulty - clean) with the largest s <= 1 that keeps the edit within `size` (half of the old atol) -> (array, s)"""
    delta = faulty - clean
    s = min(1.0, size / float(np.abs(delta).max()))
    return clean + s * delta, s


def _both(got, ref, k, what):
    msg = _rejected(got, ref) or ""
    assert ("%s: " % k) + what in msg, (k, what, msg)
    assert old_metric_accepts(got, ref), k


def test_fault_one_block_of_out_shifted():
    got, ref, _ = _clean("a")
    got["out"][3, 0:16, 64:96] += 3e-5
    _both(got, ref, "out", "step 3 block (0, 2)")


def test_fault_one_block_of_hx1_is_the_previous_steps():
    """unscaled the elementwise metric - had the suite applied it to hx1, which it never read - sees it (a state moves by ~1e-1 per step); the form
    scaled into the tolerance is accepted by it and rejected per block"""
    got, ref, _ = _clean("a")
    clean = got["hx1"][4, :, 32:64].copy()
    got["hx1"][4, :, 32:64] = got["hx1"][3, :, 32:64]
    assert "hx1: step 4 block (0, 1)" in (_rejected(got, ref) or "")
    assert not old_metric_accepts(got, ref)                    # gross: seen, where the metric is applied to the buffer at all
    assert old_metric_accepts({k: v for k, v in got.items() if k in ("out", "r_out", "n_out")}, ref)      # ... which the suite did not do
    got["hx1"][4, :, 32:64], s = _into_tolerance(clean, got["hx1"][3, :, 32:64])
    assert s < 1e-2
    _both(got, ref, "hx1", "step 4 block (0, 1)")


def test_fault_one_row_group_of_sd_h_r_is_its_neighbours():
    """rows 16..31 of step 2 take rows 32..47 (case d: 70 rows); unscaled it is gross enough for the elementwise metric, the scaled form is kept"""
    got, ref, _ = _clean("d")
    clean, other = got["sd_h_r"][2, 16:32].copy(), got["sd_h_r"][2, 32:48].copy()
    got["sd_h_r"][2, 16:32] = other
    assert "sd_h_r: step 2 block (1, 0)" in (_rejected(got, ref) or "") and not old_metric_accepts(got, ref)
    got["sd_h_r"][2, 16:32], s = _into_tolerance(clean, other)
    assert s < 1e-2
    msg = _rejected(got, ref) or ""
    assert "sd_h_r: step 2 block (1, 0)" in msg and "(2 of " in msg             # both column blocks of that row group, no other block
    assert old_metric_accepts(got, ref)


def test_fault_the_bias_missing_from_one_block_of_logits():
    """unscaled (a bias of up to 1 / sqrt(H) = 0.125) the elementwise metric sees it; the scaled form is kept"""
    got, ref, eng = _clean("a")
    bias = eng.p["linear_out_g.bias"].numpy()[32:64]
    clean = got["logits"][2, :, 32:64].copy()
    got["logits"][2, :, 32:64] = clean - bias
    assert "logits: step 2 block (0, 1)" in (_rejected(got, ref) or "") and not old_metric_accepts(got, ref)
    got["logits"][2, :, 32:64], s = _into_tolerance(clean, clean - bias)
    assert s < 1e-2
    _both(got, ref, "logits", "step 2 block (0, 1)")


def test_fault_a_non_zero_in_the_pad_columns_of_logits():
    got, ref, _ = _clean("a")
    assert (got["logits_pad"] == 0).all()
    got["logits_pad"][1, 3, 4] = 1e-7
    _both(got, ref, "logits_pad", "step 1 block (0, 0) is exactly zero in float64")


def test_fault_mu_n_of_one_block_from_the_forward_state_twice():
    """rows 16..31 of mu_n from [h_fwd | h_fwd] instead of [h_fwd | h_rev] (case d); unscaled the elementwise metric sees it, the scaled form is kept"""
    got, ref, eng = _clean("d")
    H = eng.H
    W, b = eng.p["mu_n.weight"].numpy().astype(np.float64), eng.p["mu_n.bias"].numpy().astype(np.float64)
    hf = got["enc_h_n"][16:32].astype(np.float64)
    wrong = (hf @ W[:, :H].T + hf @ W[:, H:].T + b).astype(np.float32)
    clean = got["mu_n"][16:32].copy()
    got["mu_n"][16:32] = wrong
    assert "mu_n: step 0 block (1, 0)" in (_rejected(got, ref) or "") and not old_metric_accepts(got, ref)
    got["mu_n"][16:32], s = _into_tolerance(clean, wrong)
    assert s < 1e-2
    _both(got, ref, "mu_n", "step 0 block (1, 0)")


def test_fault_a_posterior_class_flipped_and_a_missing_output():
    got, ref, _ = _clean("a")
    got["y_n"][5] ^= 1
    assert "y_n: row 5" in (_rejected(got, ref) or "")
    got, ref, _ = _clean("a")
    got["z_r"][2, 7] = np.nan
    assert "z_r: step 0 block (0, 0)" in (_rejected(got, ref) or "")
    del got["z_r"]
    with pytest.raises(AssertionError):
        check_forward_outputs(got, ref)
