"""CPU half of DESIGN 11h (the large-batch GRU cell per tile against float64): the hand plan of tests/helpers_cell.py equals fn_gru_cell_plan for every case and
every case reaches the instance it is named for; the table reaches every built instance, every (table, row constant) form of every family and both outcomes of
Stage::can_fast in both phases of the staged kernel; the input conditions hold (asserted inside cell_references); the checker accepts the float32 restatement
and, for bf16 x 6 cases, the restatement of that arithmetic; and it rejects planted faults - among them each of the six piece products dropped in its pass,
which the whole-tensor 2e-5 metric of tests/test_gpu_parity.py accepts."""
import numpy as np
import pytest
import torch

from helpers_cell import (BUILT_INSTANCES, CELL_BY_ID, CELL_CASES, CELL_F, CELL_GROUPS, CELL_V, FAMILIES, PIECE_PASSES, assert_plan_is_the_cases,
                          assert_plan_is_the_librarys, cell_case_plan, cell_reference, cell_references, cell_tile_ratio, cell_x6_restate, library_plan,
                          nominal_addresses, old_metric_accepts)
from helpers_gemm_x6 import PASS_OF_PRODUCT, PRODUCT_NAMES, split3

FAULT_MARGIN = 4            # a planted piece-product fault must put a tile at >= 4 x the bound
# the products of a low piece: 2^-16 of the pre-activation's terms - what the whole-tensor 2e-5 lets through.  mid*hi, hi*mid (2^-8) and hi*hi are far above it
SMALL_PRODUCTS = ("lo*hi", "hi*lo", "mid*mid")


def test_hand_plan_is_the_librarys_and_every_case_reaches_its_instance():
    for case in CELL_CASES:
        addr = nominal_addresses(case)
        plan = cell_case_plan(case, addr)
        assert_plan_is_the_librarys(case, plan, library_plan(case, addr))
        assert_plan_is_the_cases(case, plan)
        if case["group"] in ("views", "tiles", "ktails", "forms", "tokens") and not case["x6"]:
            assert plan["forced_honoured"], case["id"]
    # the same shapes on other offsets: an operand 4, 8 or 12 bytes into its allocation sends every LDS-free family to the staged default
    for case in (CELL_BY_ID["tiles-v5-direct-2-4-0-B81-K64"], CELL_BY_ID["tiles-v10-wlds-2-4-0-B145-K64"], CELL_BY_ID["tiles-x6-B128-H64"]):
        for name in ("x", "wih", "h", "whh", "bhh"):
            for off in (1, 2, 3):
                moved = dict(case, off={name: off}, want=("staged", (64, 2, 2)), honoured=False)
                plan = cell_case_plan(moved)
                assert_plan_is_the_librarys(moved, plan, library_plan(moved, nominal_addresses(moved)))
                assert_plan_is_the_cases(moved, plan)


def test_the_table_reaches_every_instance_form_and_load_path():
    plans = [cell_case_plan(c) for c in CELL_CASES]
    got = {(p["family"],) + tuple(p["template"]) for p in plans}
    assert got == set(BUILT_INSTANCES) | {("x6", 0, 0, 0)}, got ^ (set(BUILT_INSTANCES) | {("x6", 0, 0, 0)})
    forms = {(p["family"], p["has_tab"], p["has_rb"]) for p in plans}
    assert forms == {(f, t, r) for f in FAMILIES for t in (0, 1) for r in (0, 1)}
    no_bih = {p["family"] for c, p in zip(CELL_CASES, plans) if not c["bih"]}
    assert no_bih == set(FAMILIES)
    assert {p["fast_x"] for p in plans if p["family"] == "staged"} >= {True, False} and {p["fast_h"] for p in plans if p["family"] == "staged"} == {True, False}
    # the automatic branches, the token sources, the views, the trip counts of the bf16 x 6 producers
    auto = {(p["family"],) + tuple(p["template"]) for c, p in zip(CELL_CASES, plans) if c["variant"] == 0 and not c["x6"] and c["B"] > 512}
    assert auto == {("wlds", 2, 4, 0), ("wlds", 3, 2, 0), ("direct", 4, 2, 0), ("direct", 2, 4, 0), ("wlds-overlap", 2, 2, 0), ("wlds-overlap", 3, 2, 0),
                    ("wlds-overlap", 4, 2, 0)}
    for fam in FAMILIES:
        mine = [c for c, p in zip(CELL_CASES, plans) if p["family"] == fam]
        assert {c["tok"] for c in mine if c["tab"]} == {"idx", "start", "best"}, fam
        assert {(n, v) for c in mine for n, v in c["pad"].items() if len(c["pad"]) == 1} >= {(n, v) for n in ("x", "h", "wih", "whh", "out") for v in (4, 16)}, fam
        assert {tuple(sorted(c["pad"].items())) for c in mine if len(c["pad"]) == 5} == {tuple(sorted((n, v) for n in ("x", "h", "wih", "whh", "out"))) for v in (4, 16)}
    nblk = {(c["K1"] + c["H"]) // 32 for c, p in zip(CELL_CASES, plans) if p["family"] == "x6" and c["mode"] == "normal"}
    assert nblk >= set(range(2, 14)) | {32}
    assert {((c["K1"] + c["H"]) // 32, c["mode"]) for c in CELL_CASES if c["group"] == "x6-pieces"} == {(n, m) for n in (2, 3, 4, 32) for m in PIECE_PASSES}
    # the 4 x 8 super-tile branch of gru_cell_kernel: ntm % 4 == 0 and nut % 8 == 0
    assert any(p["family"] == "staged" and -(-c["B"] // p["template"][0]) % 4 == 0 and (c["H"] // 32) % 8 == 0 for c, p in zip(CELL_CASES, plans))
    # u0 > 0 in every K-tail case of the 32-unit families
    assert all(c["H"] >= 64 for c in CELL_CASES if c["group"] == "ktails")


@pytest.mark.parametrize("group", CELL_GROUPS)
def test_checker_accepts_the_restatements(group):
    """the input conditions (inside cell_references), the float32 restatement at a ratio <= 1 by construction, the bf16 x 6 restatement within CELL_F"""
    for case in (c for c in CELL_CASES if c["group"] == group):
        ref = cell_references(case)
        r, _, _, n = cell_tile_ratio(case, ref["fake32"], 1.0)
        assert r <= 1.0 and n == 0, (case["id"], r)
        if cell_case_plan(case)["family"] == "x6":
            r, i, j, n = cell_tile_ratio(case, cell_x6_restate(ref["inp"]), CELL_F["x6"])
            assert r <= CELL_F["x6"] and n == 0, (case["id"], r, i, j)


def test_piece_passes_hold_the_pieces_they_are_named_for():
    """A3: batch rows with three non-zero pieces, weights with one; B3 the mirror image; AB2 two and two; small one and one"""
    want = {"small": (1, 1), "A3": (3, 1), "B3": (1, 3), "AB2": (2, 2)}
    for case in (c for c in CELL_CASES if c["group"] == "x6-pieces"):
        inp = cell_references(case)["inp"]
        A = inp["h_prev"].numpy() if inp["x"] is None else np.concatenate([inp["x"].numpy(), inp["h_prev"].numpy()], 1)
        W = inp["w_hh"].numpy() if inp["x"] is None else np.concatenate([inp["w_ih"].numpy(), inp["w_hh"].numpy()], 1)
        na = max(i + 1 for i, p in enumerate(split3(A, False)) if p.any())
        nw = max(i + 1 for i, p in enumerate(split3(W, True)) if p.any())
        assert (na, nw) == want[case["mode"]], (case["id"], na, nw)
        assert float(np.abs(A).max()) <= 1.0, case["id"]


def _drop(product, rows):
    def hook(blk, c, dot):
        if c == product:
            dot = dot.copy()
            dot[rows] = 0.0
        return dot
    return hook


def _faults():
    """(name, case, faulted h_out [B][H]) of every planted fault"""
    out = []
    nan = float("nan")

    def add(name, cid, **kw):
        case = CELL_BY_ID[cid]
        out.append((name, case, cell_reference(cell_references(case)["inp"], torch.float32, **kw)))

    inp = cell_references(CELL_BY_ID["ktail-v5-H64-K80"])["inp"]
    x = inp["x"].clone()
    x[16:32, 16:32] = 0.0
    add("one k step of 16 dropped in one row tile", "ktail-v5-H64-K80", x_mm=x)
    inp = cell_references(CELL_BY_ID["ktail-v10-H288-K0"])["inp"]
    h = inp["h_prev"].clone()
    h[:, 272:] = 0.0
    add("the last ring leftover dropped", "ktail-v10-H288-K0", h_mm=h)
    inp = cell_references(CELL_BY_ID["tiles-v5-direct-2-4-0-B81-K64"])["inp"]
    x = inp["x"].clone()
    x[-1] = nan                                                             # the allocated row behind the batch
    add("a row past B read in place of the clamped row", "tiles-v5-direct-2-4-0-B81-K64", x_mm=x)
    inp = cell_references(CELL_BY_ID["form-staged-tab0-rb0-bih0"])["inp"]
    add("b_ih taken as b_hh when absent", "form-staged-tab0-rb0-bih0", b_ih=inp["b_hh"])
    case = CELL_BY_ID["x6-B128-H64-K64-nblk4"]
    out.append(("n_h fed the input blocks", case, cell_x6_restate(cell_references(case)["inp"], nh_sees_x=True)))
    case = CELL_BY_ID["token-direct-best"]
    inp = dict(cell_references(case)["inp"])
    table = torch.full_like(inp["table"], nan)
    used = torch.unique(inp["tok"])
    table[used] = inp["table"][used]
    inp.update(table=torch.cat([table, torch.full((1, table.shape[1]), nan)]), tok=inp["tok"] + 1)       # best_v - col: one row further, unselected or past the table
    out.append(("token decoded as best_v - col", case, cell_reference(inp, torch.float32)))
    inp = cell_references(CELL_BY_ID["view-direct-x-ld+4"])["inp"]
    add("one padding column read", "view-direct-x-ld+4", x_mm=torch.cat([inp["x"], torch.full((inp["x"].shape[0], 1), nan)], 1),
        w_ih=torch.cat([inp["w_ih"], torch.full((inp["w_ih"].shape[0], 1), nan)], 1))
    for case in (c for c in CELL_CASES if c["group"] == "x6-pieces"):
        inp = cell_references(case)["inp"]
        for c, name in enumerate(PRODUCT_NAMES):
            if PASS_OF_PRODUCT[name] == case["mode"]:
                out.append(("piece product %s dropped (%s, nblk %d)" % (name, case["mode"], (case["K1"] + case["H"]) // 32), case,
                            cell_x6_restate(inp, hook=_drop(c, slice(None)))))
    return out


def test_planted_faults_are_rejected_and_the_old_metric_lets_the_piece_products_through(capsys):
    """every planted fault leaves the bound; the six piece-product faults by a factor of at least FAULT_MARGIN while the whole-tensor metric accepts them"""
    lines, bad = [], []
    for name, case, got in _faults():
        ref = cell_references(case)
        F = CELL_F[cell_case_plan(case)["family"]]
        r, i, j, n = cell_tile_ratio(case, got, F)
        old = old_metric_accepts(got, ref["fake32"])
        lines.append("%-72s %-36s new: %10.1f x bound in tile (%d, %d), %d tiles  old metric: %s" % (name, case["id"], r / F, i, j, n, "accepts" if old else "rejects"))
        if not r > F:
            bad.append("not rejected: " + lines[-1])
        if name.startswith("piece product"):
            if not r >= FAULT_MARGIN * F:
                bad.append("margin below %d: %s" % (FAULT_MARGIN, lines[-1]))
            if not old and name.split()[2] in SMALL_PRODUCTS:
                bad.append("the old metric rejects: " + lines[-1])
            unfaulted = cell_tile_ratio(case, cell_x6_restate(ref["inp"]), F)
            assert unfaulted[0] <= F, (case["id"], unfaulted)
    with capsys.disabled():
        print()
        print("\n".join(lines))
    assert not bad, "\n".join(bad)


def test_a_truncated_weight_cut_cannot_be_seen_in_the_b3_pass():
    """A finding about the passes, not about the kernel: with the weights cut truncated instead of rounded the three pieces still sum to the weight exactly,
    the batch rows of the B3 pass have one piece, so no product of the nine is dropped - the accumulators, and so h_out, are the same bits.  In the other
    passes the two cuts differ in dropped products of 2^-24 of a term, below float32.  No output check can plant this fault; the split is asserted on the
    pieces instead (helpers_gemm_x6.split3 against fn_split's rounding, test_gemm_x6_reference.py)."""
    for case in (c for c in CELL_CASES if c["group"] == "x6-pieces" and c["mode"] == "B3"):
        inp = cell_references(case)["inp"]
        assert torch.equal(cell_x6_restate(inp, w_rounded=False).view(torch.int32), cell_x6_restate(inp).view(torch.int32)), case["id"]
        W = inp["w_hh"].numpy()
        assert any((a != b).any() for a, b in zip(split3(W, True), split3(W, False))), case["id"]           # ... although the pieces do differ


def test_a_nan_fails_the_bound():
    case = CELL_BY_ID["form-direct-tab1-rb1-bih1"]
    got = cell_references(case)["fake32"].clone()
    got[40, 33] = float("nan")
    r, i, j, n = cell_tile_ratio(case, got, 16)
    assert r == float("inf") and (i, j, n) == (2, 2, 1)


def test_token_words_decode_to_the_idx_tokens():
    """the host-built packed words of the idx_best cases name the tokens of the idx form: FakeOps.gru_cell gives the same bits through either"""
    from fake_ops import FakeOps
    from helpers_cell import cell_buffers
    case = CELL_BY_ID["token-staged-best"]
    outs = []
    for c in (case, dict(case, tok="idx")):
        kw, obuf = cell_buffers(c)
        h_out = kw.pop("h_out")
        FakeOps().gru_cell(kw.pop("h_prev"), kw.pop("w_hh"), kw.pop("b_hh"), h_out, **kw)
        outs.append(obuf.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    words = cell_buffers(case)[0]["idx_best"]
    assert bool((words >> 32 != 0).all()) and int(words[0] & 0xffffffff) == CELL_V - 1 and int(words[1] & 0xffffffff) == 0
