"""CPU self-test of the per-step scan checker (helpers.check_scan_vs_f64) that test_gpu_parity.test_scans_every_step_vs_fp64 applies to the HIP
scan kernels: the fp32 FakeOps stands in for the kernel, at the same T and H as the GPU cases and on the checked rows only.

It shows that the unmodified FakeOps passes on every GPU case's inputs, that those inputs satisfy the checker's input condition, that the
checker rejects planted faults the whole-tensor metric cannot see, and that the autograd reference and the hand-derived backward of FakeOps
agree in float64.  The planted faults are edits of CPU arrays.
"""
import copy

import numpy as np
import pytest
import torch

from fake_ops import FakeOps
from helpers import (SCAN_BWD_QUANTITIES, SCAN_CASES, SCAN_F, SCAN_F_CAP, SCAN_INPUTS, case_forward_only, case_kernel, check_scan_vs_f64, lib_scan_candidates, relerr,
                     run_scans, scan_inputs,
                     scan_kernel_candidates, scan_kernel_names,
                     scan_reference_f64, scan_references, scan_rows, scan_step_errors)


def _fake(name, **kw):
    """deep copy of the cached FakeOps outputs of a case (or a fresh run with keywords)"""
    scans, rows, chunk = scan_inputs(name)
    if kw:
        return run_scans(FakeOps(), kw.pop("scans", scans), rows, chunk=chunk, **kw)
    return copy.deepcopy(scan_references(scans, rows, chunk, key=name)[1])


def _check(name, got, F=None):
    scans, rows, chunk = scan_inputs(name)
    return check_scan_vs_f64(scans, got, rows, chunk, key=name, F=F)


def test_factor_is_within_its_cap():
    assert SCAN_F <= SCAN_F_CAP == 16 and SCAN_F & (SCAN_F - 1) == 0


@pytest.mark.parametrize("name", sorted(SCAN_INPUTS))
def test_fake_ops_passes_and_inputs_satisfy_the_condition(name):
    """the fp32 restatement passes its own check (ratio 1 by construction) on every GPU case's inputs; scan_references asserts the input condition:
    every per-step block maximum of the fp64 reference >= 2**-100, every e_ref finite and non-zero.  A forward-only scan (gates=False) has h_all alone."""
    worst = _check(name, _fake(name), F=1)
    scans = scan_inputs(name)[0]
    for i, s in enumerate(scans):
        want = set(("h_all", "gate_r", "gate_z", "gate_n", "gate_hn", "dgx_all", "dghn_all"))
        want |= {"dh0"} if s.get("want_dh0") else set()
        want |= {"dgx_rowsum", "dghn_rowsum"} if s.get("want_rowsums", True) else set()
        if not s.get("gates", True):
            want = {"h_all"}
        assert {k for (j, k) in worst if j == i} == want, (i, sorted(worst))
    assert all(v[0] <= 1.0 for v in worst.values())


def test_every_gpu_case_names_inputs_and_reaches_its_kernels():
    """the shapes of the case table reach the kernel instances the cases are meant for (the dispatch restated by scan_kernel_names), first and tail
    chunk of a chained case alike, and together they name every instance fn_gru_seq_fwd / fn_gru_seq_bwd can launch"""
    seen = set()
    for c in SCAN_CASES:
        scans, rows, chunk = scan_inputs(c["inputs"])
        Ts = [None] if chunk is None else sorted({chunk, scans[0]["T"] % chunk or chunk})
        for T in Ts:
            names = scan_kernel_names(scans, c["variants"], c["x6"], c["budget"], c["persistent"], T=T)
            seen.update(names)
            for i, got in enumerate(names):
                want = case_kernel(c, i, T)
                assert want is None or want == got, (c["id"], T, want, got)
            if case_forward_only(c):
                assert case_kernel(c, 0, T) is not None and c["kernels"][1] is None and not names[0].startswith(("gru_fwd_pp", "gru_fwd_x6")), (c["id"], names)
    tilings = ("4, 1, 2", "4, 1, 1", "2, 2, 2", "2, 2, 1", "1, 4, 1")
    every = {"gru_fwd_x6pp_kernel<1>", "gru_fwd_x6pp_kernel<2>", "gru_fwd_x6_kernel<1>", "gru_fwd_x6_kernel<2>", "gru_fwd_pp_kernel<1>", "gru_fwd_pp_kernel<2>",
             "gru_bwd_x6_kernel<1>", "gru_bwd_x6_kernel<2>", "gru_bwd_rs_kernel<1>", "gru_bwd_rs_kernel<2>", "gru_fwd_step_kernel", "gru_bwd_step_kernel"}
    every |= {"gru_fwd_persist_kernel<%s, 4>" % t for t in tilings} | {"gru_bwd_persist_kernel<%s, 8>" % t for t in tilings}
    assert every <= seen, sorted(every - seen)
    assert len({c["id"] for c in SCAN_CASES}) == len(SCAN_CASES)


def test_restated_dispatch_is_the_librarys_on_every_gpu_case():
    """scan_kernel_candidates (the hand restatement the case table is checked with) against fn_gru_fwd_plan / fn_gru_bwd_plan at 256 compute units:
    the same candidates in the same order for every case, first and tail chunk, aligned and with a misaligned epilogue operand"""
    for c in SCAN_CASES:
        scans, rows, chunk = scan_inputs(c["inputs"])
        for T in [None] if chunk is None else sorted({chunk, scans[0]["T"] % chunk or chunk}):
            for aligned in ((True, True), (False, True), (True, False)):
                kw = dict(variants=c["variants"], x6=c["x6"], cu_budget=c["budget"], persistent=c["persistent"], T=T, cus=256, aligned=aligned)
                assert scan_kernel_candidates(scans, **kw) == lib_scan_candidates(scans, **kw), (c["id"], T, aligned)


def test_a_forward_only_launch_is_refused_the_bf16x6_kernels():
    """gates = NULL and the bf16 x 6 arithmetic asked for: the library refuses the call (no candidate, FN_E_UNSUPPORTED) and the restatement returns [] -
    at every forward-only case, first and tail chunk; the same shapes WITH gates are taken where the case has 64-row groups at hidden 512.  The engine
    asks fn_gru_fwd_x6_ok first and therefore runs a save=False pipeline on fp32."""
    fo = [c for c in SCAN_CASES if case_forward_only(c)]
    assert {c["inputs"] for c in fo} == {"fo_enc", "fo_dec", "fo_33_96", "fo_200_64", "fo_step"}
    for c in fo:
        scans, rows, chunk = scan_inputs(c["inputs"])
        for T in [None] if chunk is None else sorted({chunk, scans[0]["T"] % chunk or chunk}):
            kw = dict(variants=c["variants"], x6=True, persistent=c["persistent"], T=T, cus=256)
            assert scan_kernel_candidates(scans, **kw)[0] == [] == lib_scan_candidates(scans, **kw)[0], (c["id"], T)
    for name, T in (("fo_enc", None), ("fo_dec", 2)):
        gated = [dict(s, gates=True) for s in scan_inputs(name)[0]]
        mine = scan_kernel_candidates(gated, x6=True, T=T)[0]
        assert mine == lib_scan_candidates(gated, x6=True, T=T)[0] and mine and mine[0].startswith("gru_fwd_x6"), (name, mine)


def test_restated_dispatch_is_the_librarys_on_a_seeded_sweep():
    """the same over 4000 seeded descriptor sets drawn from the value sets of csrc/host/gru_plan_check.cpp: 1-8 scans, mostly of one B / H / T, every
    variant bit and forced row block, compute units, budgets, alignment, gates and input sources present or absent"""
    import random
    rng = random.Random(20260)
    Bs, Hs, Ts = (1, 16, 31, 32, 33, 64, 128, 200, 256, 512), (32, 64, 96, 512, 544), (1, 2, 3, 70)
    bits = (0, 0, 0, 0, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x8000)
    seen = set()
    for i in range(4000):
        n = rng.randint(1, 8)
        B, H, T = rng.choice(Bs), rng.choice(Hs + (512, 512)), rng.choice(Ts)
        if i % 8 == 0:                                         # the production launches: 8 - 16 full row groups at H = 512
            (n, B), H, T = rng.choice(((4, 256), (2, 256), (2, 512), (1, 512), (8, 64), (3, 256))), 512, 70
        scans = []
        for _ in range(n):
            s = dict(B=B if rng.random() < 0.9 else rng.choice(Bs), H=H if rng.random() < 0.98 else rng.choice(Hs), T=T if rng.random() < 0.9 else rng.choice(Ts))
            src = rng.choice(("table", "table", "dense", "both"))
            s.update({k: True for k in (("gx_table",) if src == "table" else ("gx_dense",) if src == "dense" else ("gx_table", "gx_dense"))})
            s["gates"] = rng.random() < 0.95
            scans.append(s)
        kw = dict(variants=tuple(rng.choice(bits) | rng.choice(bits) | rng.choice((0, 0, 0, 0, 16, 32, 64, 128, 5)) for _ in range(2)), x6=rng.random() < 0.3,
                  cu_budget=(rng.choice((0, 128)), rng.choice((0, 128))), persistent=rng.random() < 0.95, cus=rng.choice((16, 31, 32, 128, 248, 256, 304)),
                  aligned=(rng.random() < 0.9, rng.random() < 0.9))
        if i % 8 == 0:
            kw.update(variants=(rng.choice((0, 0x8000)), rng.choice((0, 0x8000))), x6=rng.random() < 0.5, cus=rng.choice((256, 304)), aligned=(True, True))
        mine, theirs = scan_kernel_candidates(scans, **kw), lib_scan_candidates(scans, **kw)
        assert mine == theirs, (i, scans, kw, mine, theirs)
        seen.update(mine[0] + mine[1])
    from music_fader_nets_amd import _lib
    assert seen == set(_lib.GRU_PLAN_KERNELS), sorted(set(_lib.GRU_PLAN_KERNELS) - seen)


def test_scan_plan_kernel_names_follow_the_header_enum():
    import ctypes
    import os
    import re
    from mfn_import import ROOT, load_package
    load_package()
    from music_fader_nets_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fadernets.h")).read()
    names = re.findall(r"^\s*(FN_GRU_(?:FWD|BWD)_[A-Z0-9_]+)", hdr.split("enum FnGruKernel {")[1].split("};")[0], re.M)
    assert len(names) == len(_lib.GRU_PLAN_KERNELS) == 22

    def kernel_name(n):
        d, rest = n[len("FN_GRU_"):].lower().split("_", 1)
        if rest == "step":
            return "gru_%s_step_kernel" % d
        if rest.startswith("ws_"):
            return "gru_%s_persist_kernel<%s, %d>" % (d, rest[3:].replace("_", ", "), 8 if d == "bwd" else 4)
        fam, t = rest.rsplit("_", 1)
        return "gru_%s_%s_kernel<%s>" % (d, fam, t)
    assert tuple(kernel_name(n) for n in names) == _lib.GRU_PLAN_KERNELS
    src = open(os.path.join(ROOT, "music-fader-nets_amd", "csrc", "gru_persist.hip")).read() + open(os.path.join(ROOT, "music-fader-nets_amd", "csrc", "gru.hip")).read()
    for k in _lib.GRU_PLAN_KERNELS:
        assert re.search(r"\b%s\b" % k.split("<")[0], src), k
    lib, plan = _lib.load(), _lib.FnGruPlan()
    assert lib.fn_gru_fwd_plan(None, 1, 256, None) == _lib.FN_E_NULL and lib.fn_gru_bwd_plan(None, 1, 256, None) == _lib.FN_E_NULL
    assert lib.fn_gru_fwd_plan(None, 1, -1, ctypes.byref(plan)) == _lib.FN_E_SHAPE and lib.fn_gru_bwd_plan(None, 1, -1, ctypes.byref(plan)) == _lib.FN_E_SHAPE
    assert lib.fn_gru_fwd_plan(None, 1, 256, ctypes.byref(plan)) == 0 and plan.status == _lib.FN_E_NULL and plan.n == 0
    assert lib.fn_gru_cell_plan(None, None) == _lib.FN_E_NULL


@pytest.mark.parametrize("B", [65, 200, 256, 512, 33, 1])
def test_scan_rows_hits_every_16_row_tile_twice(B):
    for seed in range(5):
        rows = scan_rows(B, seed)
        assert len(set(rows.tolist())) == len(rows) and rows.min() >= 0 and rows.max() < B
        for r0 in range(0, B, 16):
            n = min(16, B - r0)
            hit = [r for r in rows if r0 <= r < r0 + n]
            assert r0 in hit and len(hit) >= min(2, n), (B, seed, r0, hit)
    if B <= 64:
        assert np.array_equal(scan_rows(B), np.arange(B))
    else:
        assert not np.array_equal(scan_rows(B, 0), scan_rows(B, 1))


def _rejects(name, got, what):
    with pytest.raises(AssertionError) as e:
        _check(name, got)
    assert what in str(e.value), str(e.value)
    return str(e.value)


def test_fault_1_a_patch_at_an_early_step_of_a_dh_last_only_scan():
    """a 16-row x 32-column patch of dgx_all at step 40 of the 256-step encoder shape x (1 + 1e-3): the whole-tensor metric at 5e-5 does not see
    it (the gate gradients of step 40 are ~2**-100 of the last step's), the per-step metric rejects it"""
    scans, rows, chunk = scan_inputs("enc")
    got = _fake("enc")
    ref64 = scan_references(scans, rows, chunk, key="enc")[0]
    clean = relerr(got[1]["dgx_all"].numpy(), ref64[1]["dgx_all"].numpy())
    tile = torch.from_numpy(np.nonzero((rows[1] // 16) == 5)[0])         # the checked rows of the 16-row tile 80..95
    assert len(tile) == 2
    got[1]["dgx_all"][40, tile, 512 + 64:512 + 96] *= 1 + 1e-3
    blind = relerr(got[1]["dgx_all"].numpy(), ref64[1]["dgx_all"].numpy())
    assert blind < 5e-5 and blind == clean, (blind, clean)               # the old metric: unchanged to the last digit
    msg = _rejects("enc", got, "scan 1 dgx_all")
    assert "at step 40, row block 0" in msg, msg
    err = scan_step_errors(got, ref64, rows)[(1, "dgx_all")][0][40, 0]
    e_ref = scan_references(scans, rows, chunk, key="enc")[2][(1, "dgx_all")][0][40, 0]
    assert err > SCAN_F_CAP * max(e_ref, 2.0 ** -23), (err, e_ref)        # rejected for any F up to the cap


@pytest.mark.parametrize("kind", ["dropped", "scaled"])
def test_fault_2_the_carry_between_two_backward_chunks(kind):
    """the state gradient that leaves backward chunk 3 of the decoder-pipeline chain dropped, or x (1 + 1e-4)"""
    def fault(ci, carry):
        if ci == 3:
            carry.zero_() if kind == "dropped" else carry.mul_(1 + 1e-4)
    _rejects("dec", _fake("dec", carry_fault=fault), "dgx_all")


def test_fault_3_the_token_of_a_reverse_scan_off_by_one_step():
    scans = [dict(s) for s in scan_inputs("enc")[0]]
    scans[3]["idx"] = torch.roll(scans[3]["idx"], 1, dims=1)
    msg = _rejects("enc", _fake("enc", scans=scans), "scan 3 h_all")
    assert "scan 0" not in msg and "scan 1 " not in msg and "scan 2" not in msg


def test_fault_4_r_and_z_planes_of_the_saved_gates_swapped_at_one_step():
    got = _fake("attr")
    r = got[0]["gate_r"][17].clone()
    got[0]["gate_r"][17] = got[0]["gate_z"][17]
    got[0]["gate_z"][17] = r
    msg = _rejects("attr", got, "scan 0 gate_r")
    assert "scan 0 gate_z" in msg and "at step 17" in msg


def test_fault_5_dghn_of_one_step_without_the_factor_r():
    got = _fake("dec")
    got[1]["dghn_all"][200] = got[1]["dghn_all"][200] / got[1]["gate_r"][200]
    msg = _rejects("dec", got, "scan 1 dghn_all")
    assert "at step 200" in msg


def test_a_nan_or_a_missing_output_is_rejected():
    got = _fake("t2")
    got[0]["dh0"][3, 7] = float("nan")
    _rejects("t2", got, "scan 0 dh0")
    got = _fake("t2")
    del got[1]["dghn_rowsum"]
    _rejects("t2", got, "dghn_rowsum missing")


@pytest.mark.parametrize("name", ["eight", "ws_33_96", "dec_tail"])
def test_autograd_reference_agrees_with_the_hand_derived_backward_in_float64(name):
    """the one place where FakeOps.gru_seq_bwd (the gate-gradient algebra the kernels implement) and torch autograd through the fp64 forward are
    pinned to each other: FakeOps on float64 tensors (under the float64 default dtype, as helpers.oracle_grads_f64 does it), every step of every
    output within 1e-12 of the block maximum"""
    scans, rows, chunk = scan_inputs(name)
    if name == "dec_tail":
        rows = [r[:8] for r in rows]
    ref64 = scan_reference_f64(scans, rows)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        s64 = [{k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in s.items()} for s in scans]
        got = run_scans(FakeOps(), s64, rows, chunk=chunk)
    finally:
        torch.set_default_dtype(old)
    assert all(v.dtype == torch.float64 for o in got for v in o.values())
    n = 0
    for (i, k), (e, den) in scan_step_errors(got, ref64, rows).items():
        assert e.max() < 1e-12, (i, k, e.max())
        n += k in SCAN_BWD_QUANTITIES
    assert n >= 4 * len(scans) - 8
