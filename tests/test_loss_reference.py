"""CPU self-test of tests/helpers_loss.py, the case tables, float64 references and checkers that tests/test_gpu_loss.py applies to the loss-head
kernels of csrc/loss.hip.  tests/fake_ops.FakeOps (torch.log_softmax) and helpers_loss.StepOps (the documented steps in float32) stand in for the
kernels, through the same drivers.

It shows that the tables have the properties their ids claim, that the input conditions hold for every case, that the float64 references are the
gradients autograd gives for the documented losses, that every checker accepts both stand-ins on every case, and that every planted fault - an edit of
the float32 restatement - is rejected, one of which the whole-tensor close(..., 2e-5) of test_gpu_parity.py accepts."""
import numpy as np
import pytest
import torch

from fake_ops import FakeOps
from helpers import SCAN_F_CAP
from helpers_loss import (ADV_CASES, ADV_MIN_PRE, ADV_SHAPES, ADV_ZROW, ARGMAX_B, ARGMAX_CASES, ARGMAX_E, ARGMAX_KINDS, EXACT_PASS, F32, F64, LOSS_F, MASKED_CASES,
                          MASKED_FORMS, ONEHOT_CASES, PAIR_CASES, PAIR_SHAPES, RANDN_PASS, TIME_BWD_CASES, TIME_BY_ID, TIME_CASES, TIME_SHAPES, VOCAB_BWD_CASES,
                          VOCAB_BY_ID, VOCAB_CASES, VOCAB_E, VOCAB_ROWS, StepOps, adv_inputs, adv_math, adv_references, argmax_inputs, argmax_references,
                          argmax_row_kind, assert_F, bits_equal, check_adv, check_argmax, check_masked, check_onehot, check_pair, check_quantities, check_time,
                          check_time_bwd, check_vocab, check_vocab_bwd, f32, masked_math, old_metric_accepts, onehot_inputs, pair_inputs,
                          pair_references, pairwise_math, run_adv, run_argmax, run_masked, run_onehot, run_pair, run_time, run_time_bwd, run_vocab,
                          run_vocab_bwd, time_bwd_math, time_grid, time_identity_inputs, time_identity_views, time_inputs, time_kernel, time_math,
                          vocab_bwd_math, vocab_inputs, vocab_math, vocab_references)

BACKENDS = (FakeOps, StepOps)
V342 = VOCAB_BY_ID["B7-T23-E342-ld344-all-randn3"]


def _F(backend, family):
    """LOSS_F is tightened to what the kernels measure; FakeOps is another float32 evaluation and gets the cap"""
    return SCAN_F_CAP if backend is FakeOps else LOSS_F[family]


def _ids(cases):
    return [c["id"] for c in cases]


# ---- the case tables ------------------------------------------------------------------------------------------------------------------------
def test_vocab_table_reaches_every_row_tail_and_lane_tail():
    assert [B * T % 4 for B, T in VOCAB_ROWS] == [1, 1, 3, 1, 1, 2, 0]
    assert {(c["B"], c["T"]) for c in VOCAB_CASES} == set(VOCAB_ROWS) and all(B != T and min(B, T) > 1 for B, T in ((7, 23), (5, 13), (2, 3), (4, 2)))
    assert {c["E"] for c in VOCAB_CASES if (c["B"], c["T"]) == (7, 23)} == set(VOCAB_E) == {1, 2, 63, 64, 65, 128, 129, 342, 385, 1024}
    assert [E % 64 for E in VOCAB_E] == [1, 2, 63, 0, 1, 0, 1, 22, 1, 0]
    per_lane = lambda E: [len(range(lane, E, 64)) for lane in range(64)]          # noqa: E731
    assert per_lane(342) == [6] * 22 + [5] * 42                                   # lanes 0..21 hold a sixth entry
    assert per_lane(63) == [1] * 63 + [0] and per_lane(1) == [1] + [0] * 63 and per_lane(2).count(0) == 62     # empty lanes
    assert per_lane(65) == [2] + [1] * 63 and per_lane(385)[:2] == [7, 6] and set(per_lane(1024)) == {16}
    assert all(c["ld"] == (c["E"] + 3) // 4 * 4 for c in VOCAB_CASES if c["id"] != "B7-T23-E342-ld346-all-randn3") and VOCAB_BY_ID["B7-T23-E342-ld346-all-randn3"]["ld"] == 346
    assert {c["form"] for c in VOCAB_CASES} == {"lp", "nll", "dl", "all", "alias", "gs0"} and {c["kind"] for c in VOCAB_CASES} == {"randn3", "p90", "m90", "ninf", "lowp"}
    assert VOCAB_BY_ID["B7-T23-E1-ld4-all-randn3"]["zero"] == ("logp", "nll", "dlogits") and VOCAB_BY_ID["B7-T23-E342-ld344-gs0-randn3"]["zero"] == ("dlogits",)
    assert len(VOCAB_BWD_CASES) == 21


def test_vocab_inputs_are_what_their_kind_says():
    for c in VOCAB_CASES:
        inp, B, T, E = vocab_inputs(c), c["B"], c["T"], c["E"]
        tg = inp["target"]
        assert tg.dtype == torch.int32 and tuple(tg.shape) == (B, T) and int(tg.min()) >= 0 and int(tg.max()) < E
        flat = tg.reshape(-1)
        assert bool((flat[0::7] == 0).all()) and bool((flat[1::7] == E - 1).all())
        x, row_tg = inp["x"], tg.long().t().reshape(-1)
        if c["kind"] == "ninf":
            ninf = torch.isneginf(x)
            assert bool((ninf.sum(1) == 1).all()) and not bool(ninf.gather(1, row_tg.view(-1, 1)).any())
        else:
            assert bool(torch.isfinite(x).all())
        if c["kind"] == "lowp":
            assert not bool(((tg >= 32) & (tg < 48)).any()) and float(x[:, 32:48].mean()) < -10
        if c["kind"] in ("p90", "m90"):
            m = float(x.mean())
            assert abs(abs(m) - 90) < 1 and (m > 0) == (c["kind"] == "p90")
            if c["kind"] == "p90":
                assert bool(torch.isinf(torch.exp(x).sum(1)).all())               # without the max subtraction the sum overflows
            else:
                assert float(torch.exp(x).sum(1).max()) < 2.0 ** -100             # ... or falls below the smallest tile maximum the metric admits


def test_argmax_table_plants_every_tie():
    assert ARGMAX_B == (1, 3, 4, 13) and ARGMAX_E == (1, 63, 64, 65, 342, 1024) and len(ARGMAX_CASES) == 48
    assert [B % 4 for B in ARGMAX_B] == [1, 3, 0, 1]
    assert {argmax_row_kind(13, r) for r in range(13)} == set(ARGMAX_KINDS) | {None}
    for B in ARGMAX_B:
        assert any(argmax_row_kind(B, r) is not None for r in range(B))
    for c in ARGMAX_CASES:
        rec = argmax_references(c)
        x, tok = rec["inputs"]["x"], rec["tokens"]
        for r in range(c["B"]):
            assert float(x[r, int(tok[r])]) == float(x[r].max()) and not bool((x[r, :int(tok[r])] == x[r].max()).any())
    inp = argmax_inputs(dict(B=13, E=342))
    kinds = {argmax_row_kind(13, r): r for r in range(13)}
    x = inp["x"]
    r = kinds["tie-same-lane"]
    assert float(x[r, 5]) == float(x[r, 69]) == float(x[r].max()) and 5 % 64 == 69 % 64
    r = kinds["tie-across-lanes"]
    assert float(x[r, 10]) == float(x[r, 41]) == float(x[r].max())
    r = kinds["signed-zeros"]
    assert np.signbit(x[r, 2].numpy()) and not np.signbit(x[r, 7].numpy()) and float(x[r].max()) == 0.0 and inp["expect"][r] == 2
    r = kinds["all-but-one-ninf"]
    assert int(torch.isneginf(x[r]).sum()) == 341
    assert int(torch.isneginf(x[kinds["some-ninf"]]).sum()) == 114 and inp["expect"][kinds["constant"]] == 0


def test_time_table_takes_the_kernel_it_names():
    assert set(TIME_SHAPES) == {(1, 3, 3), (2, 9, 3), (63, 9, 3), (64, 9, 3), (65, 9, 3), (70, 5, 5), (33, 9, 16), (8, 1, 16), (64, 86, 3)}
    for c in TIME_CASES:
        assert ("wave" in c["id"]) == (c["Tr"] <= 64) == (time_kernel(c["Tr"]) == "time_logsoftmax_wave_kernel")
    assert {c["Tr"] for c in TIME_CASES if "loop" in c["id"]} == {65, 70}
    assert time_grid(64, 86, 3) == (65, 2) and 86 * 3 == 258 == 256 + 2 and (258 + 255) // 256 == 2          # wave grid: 258 % 4 = 2; the bwd grid: two columns in a second workgroup
    assert time_grid(70, 5, 5) == (1, 231) and time_grid(1, 3, 3) == (3, 3)
    assert TIME_BY_ID["Tr1-B3-C3-wave-train"]["zero"] == ("logp", "nll_bc", "dlogits") and len(TIME_BWD_CASES) == 9
    for c in TIME_CASES:
        tg = time_inputs(c)["target"]
        assert tuple(tg.shape) == (c["B"], c["Tr"]) and bool((tg[0] == 0).all()) and int(tg.max()) < c["Cc"]
    case, x65 = time_identity_inputs()
    assert x65.shape[0] == 65 and bits_equal(x65[:64], time_inputs(case)["x"]) and float(x65[64].max()) == -1e4


def test_masked_pair_adv_onehot_tables():
    assert len(MASKED_CASES) == 3 * (5 + 4) and {c["ld"] - c["E"] for c in MASKED_CASES} == {2} and MASKED_FORMS == ("sums", "grad", "both", "inplace")
    for c in MASKED_CASES:
        assert all(0 <= lo <= hi <= c["E"] for lo, hi in c["ranges"])
    by = {c["range_name"]: c["ranges"] for c in MASKED_CASES if c["E"] == 342}
    assert by["reference"] == ((2, 90), (180, 278)) and by["empty"][0][0] == by["empty"][0][1] and by["full"][0] == (0, 342) and by["ends-at-E"][0][1] == 342
    (a0, a1), (b0, b1) = by["overlap"]
    assert a0 < b0 < a1 < b1
    assert set(PAIR_SHAPES) == {(1, 0, 1), (63, 0, 63), (65, 1, 64), (300, 150, 100), (300, 297, 3)} and len(PAIR_CASES) == 20
    assert [nr % 4 for _, _, nr in PAIR_SHAPES] == [1, 3, 0, 0, 3] and [n % 64 for n, _, _ in PAIR_SHAPES] == [1, 63, 1, 44, 44]
    tiny = [c for c in PAIR_CASES if c["tiny"]]
    assert len(tiny) == 4
    a = pair_inputs(tiny[0])["attr"]
    assert a.dtype == F64 and len(a.unique()) == 3 and len(a.float().unique()) == 1          # distinct in float64, one value in float32
    a = pair_inputs(PAIR_CASES[-1])["attr"]
    assert len(a.unique()) == 5 and a.numel() == 300                                          # many exact ties
    assert set(ADV_SHAPES) == {(1, 1, 1), (5, 63, 64), (37, 96, 104), (6, 128, 128), (9, 65, 72)} and len(ADV_CASES) == 20
    assert [Z % 64 for _, Z, _ in ADV_SHAPES] == [1, 63, 32, 0, 1] and [B % 4 for B, _, _ in ADV_SHAPES] == [1, 1, 1, 2, 1]
    assert {(c["rows"], c["V"]) for c in ONEHOT_CASES} == {(r, V) for r in (1, 5, 161) for V in (1, 3, 64, 65, 342)}
    kinds = set()
    for c in ONEHOT_CASES:
        oh = onehot_inputs(c)["oh"]
        for r in range(c["rows"]):
            mx = float(oh[r].max())
            kinds.add("zeros" if mx == 0 else "tie" if int((oh[r] == mx).sum()) > 1 else "onehot" if mx == 1.0 and int((oh[r] != 0).sum()) == 1 else "soft")
    assert kinds == {"zeros", "tie", "onehot", "soft"}
    assert all(0 < F <= SCAN_F_CAP for F in LOSS_F.values())
    assert LOSS_F == dict(vocab_logsoftmax=8, vocab_logsoftmax_bwd=16, vocab_argmax=1, time_logsoftmax=16, time_logsoftmax_bwd=8, masked_prob=16, pairwise_reg=2, adv_head=4)
    with pytest.raises(AssertionError):
        assert_F(2 * SCAN_F_CAP)


# ---- the input conditions -------------------------------------------------------------------------------------------------------------------
def test_adv_inputs_keep_every_gate_away_from_zero():
    for c in ADV_CASES:
        rec, inp = adv_references(c), adv_inputs(c)
        pre, B = rec["pre"], c["B"]
        planted = torch.zeros(B, 2, dtype=torch.bool)
        if B >= 5:
            planted[ADV_ZROW, 0] = True
            assert float(pre[ADV_ZROW, 0]) == 0.0 and float(inp["z"][ADV_ZROW].abs().max()) == 0.0 and float(inp["b_r"]) == 0.0
            assert bool((inp["mask"][3] == 0).all())                               # a row with both attributes masked
        assert float(pre.abs()[~planted].min()) >= ADV_MIN_PRE
        assert set(inp["mask"].unique().tolist()) <= {0.0, f32(1 / 0.7)}
        pre32 = adv_math(inp, None, None, F32)["pre"]
        assert torch.equal(pre32 > 0, pre > 0)                                     # no gate flips on rounding


def test_exact_pass_is_exact_and_signs_need_float64():
    for c in PAIR_CASES:
        rec = pair_references(c)                                                   # asserts integer sums below 2**24, fp32 == fp64
        if c["kind"] == EXACT_PASS and c["n_all"] > 1:
            assert float(rec["ref64"]["loss_rows"].max()) >= 4.0
    c = [c for c in PAIR_CASES if c["tiny"] and c["kind"] == RANDN_PASS][0]
    inp = pair_inputs(c)
    good = pairwise_math(inp["z0"], inp["attr"], c["row0"], c["nrows"], 1.0, F64)
    bad = pairwise_math(inp["z0"], inp["attr"], c["row0"], c["nrows"], 1.0, F64, fault="sign_f32")
    assert float((good["loss_rows"] - bad["loss_rows"]).abs().max()) > 1.0


# ---- the float64 references are autograd of the documented losses -------------------------------------------------------------------------------
def _agree(a, b, tol=1e-12):
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def test_references_agree_with_autograd_in_float64():
    gen = torch.Generator().manual_seed(5)
    B, T, E, gs = 3, 5, 37, 0.37
    x = (torch.randn(T * B, E, generator=gen, dtype=F64) * 3).requires_grad_(True)
    tgt = torch.randint(0, E, (B, T), generator=gen, dtype=torch.int32)
    lp = torch.log_softmax(x, 1).view(T, B, E)
    nll = -lp.gather(2, tgt.long().t().unsqueeze(-1)).reshape(-1)
    ref = vocab_math(x, tgt, B, T, gs, F64)
    _agree(ref["nll"], nll.detach()), _agree(ref["logp"].view(B, T, E), lp.detach().permute(1, 0, 2))
    _agree(ref["dlogits"], torch.autograd.grad(gs * nll.sum(), x, retain_graph=True)[0])
    g = torch.randn(B, T, E, generator=gen, dtype=F64)
    lp_bt = lp.permute(1, 0, 2)
    _agree(vocab_bwd_math(lp_bt.detach(), g, F64)["dlogits"], torch.autograd.grad((lp_bt * g).sum(), x)[0])
    # time axis: nll_bc[b][c] = - sum over the steps t with target[b][t] == c of logp[b][t][c]
    Tr, Cc = 7, 4
    x = (torch.randn(Tr, B, Cc, generator=gen, dtype=F64) * 2).requires_grad_(True)
    tgt = torch.randint(0, Cc, (B, Tr), generator=gen, dtype=torch.int32)
    lp = torch.log_softmax(x, 0)
    nll = torch.stack([torch.stack([-sum((lp[t, b, c] for t in range(Tr) if int(tgt[b, t]) == c), torch.zeros((), dtype=F64)) for c in range(Cc)]) for b in range(B)])
    ref = time_math(x, tgt, 0.11, F64)
    _agree(ref["nll_bc"], nll.detach()), _agree(ref["logp"].view(B, Tr, Cc), lp.detach().permute(1, 0, 2))
    _agree(ref["dlogits"].view(Tr, B, Cc), torch.autograd.grad(0.11 * nll.sum(), x, retain_graph=True)[0])
    g = torch.randn(B, Tr, Cc, generator=gen, dtype=F64)
    _agree(time_bwd_math(lp.detach().permute(1, 0, 2), g, F64)["dlogits"].view(Tr, B, Cc), torch.autograd.grad((lp.permute(1, 0, 2) * g).sum(), x)[0])
    # masked probability sums and the gradient of w0 P_0 + w1 P_1
    x = (torch.randn(5, 40, generator=gen, dtype=F64) * 3).requires_grad_(True)
    w, ranges = torch.randn(5, 2, generator=gen, dtype=F64), ((2, 11), (7, 40))
    p = torch.softmax(x, 1)
    P = torch.stack([p[:, 2:11].sum(1), p[:, 7:40].sum(1)], 1)
    ref = masked_math(x, ranges, w, F64)
    _agree(ref["sums"], P.detach()), _agree(ref["dlogits"], torch.autograd.grad((w * P).sum(), x)[0])
    # pairwise regulariser: dz0 = grad_scale d/dz0 of the sum over ALL ordered pairs
    z = torch.randn(9, generator=gen, dtype=F64).requires_grad_(True)
    attr = torch.randint(0, 3, (9,), generator=gen).double()
    full = ((torch.tanh(z.view(-1, 1) - z.view(1, -1)) - torch.sign(attr.view(-1, 1) - attr.view(1, -1))) ** 2)
    ref = pairwise_math(z.detach().float().double(), attr, 2, 5, 0.37, F64)
    zz = z.detach().float().double().requires_grad_(True)
    full = ((torch.tanh(zz.view(-1, 1) - zz.view(1, -1)) - torch.sign(attr.view(-1, 1) - attr.view(1, -1))) ** 2)
    _agree(ref["loss_rows"].view(-1), full.sum(1)[2:7].detach()), _agree(ref["dz0"].view(-1), torch.autograd.grad(0.37 * full.sum(), zz)[0][2:7])
    # adversarial heads: da = d/dpre of lam sum_a mean_b (o - dens)^2, g_z = g0 - dL/dz (gradient reversal)
    inp = {k: (v.double() if torch.is_tensor(v) else v) for k, v in adv_inputs(ADV_CASES[8]).items()}
    z = inp["z"].clone().requires_grad_(True)
    pre = torch.stack([z @ inp["w_r"].view(-1) + inp["b_r"].view(()), z @ inp["w_n"].view(-1) + inp["b_n"].view(())], 1)
    pre.retain_grad()
    o = torch.relu(pre) * inp["mask"]
    (0.03 * inp["inv_bg"] * ((o - inp["dens"]) ** 2).sum()).backward()
    ref = adv_math(inp, 0.03, inp["g0"], F64)
    _agree(ref["o"], o.detach()), _agree(ref["da"], pre.grad), _agree(ref["g_z"], inp["g0"] - z.grad), _agree(ref["loss_rows"], ((o - inp["dens"]) ** 2).detach())


# ---- every checker accepts FakeOps and the float32 restatement through the same drivers ---------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS, ids=lambda b: b.__name__)
def test_checkers_accept_the_stand_ins_on_every_vocab_case(backend):
    """FakeOps is torch.log_softmax: at +-90 it is the more accurate of the two, and passes a bound made of the documented steps' own error"""
    ops = backend()
    for c in VOCAB_CASES:
        w = check_vocab(c, run_vocab(ops, c), _F(backend, "vocab_logsoftmax"))
        assert w[0] <= (1.0 if backend is StepOps else SCAN_F_CAP)
        if c["form"] == "alias":
            a, b = run_vocab(ops, c), run_vocab(ops, c, form="all")
            assert bits_equal(a["dlogits"], b["dlogits"]) and bits_equal(a["logp"], b["logp"]) and bits_equal(a["nll"], b["nll"])
    for c in VOCAB_BWD_CASES:
        check_vocab_bwd(c, run_vocab_bwd(ops, c), _F(backend, "vocab_logsoftmax_bwd"))
    rec = vocab_references(VOCAB_BY_ID["B7-T23-E342-ld344-all-p90"])
    assert max(float(rec["e_ref"][k].max()) for k in ("logp", "dlogits")) > 4 * max(float(rec["e_torch"][k].max()) for k in ("logp", "dlogits"))


@pytest.mark.parametrize("backend", BACKENDS, ids=lambda b: b.__name__)
def test_checkers_accept_the_stand_ins_on_every_other_case(backend):
    ops = backend()
    for c in ARGMAX_CASES:
        check_argmax(c, run_argmax(ops, c), _F(backend, "vocab_argmax"))
    for c in TIME_CASES:
        check_time(c, run_time(ops, c), _F(backend, "time_logsoftmax"))
    for c in TIME_BWD_CASES:
        check_time_bwd(c, run_time_bwd(ops, c), _F(backend, "time_logsoftmax_bwd"))
    case, x65 = time_identity_inputs()
    a, b = time_identity_views(case, run_time(ops, case), run_time(ops, case, x=x65))
    assert bits_equal(a, b) or backend is FakeOps
    for c in MASKED_CASES:
        outs = {f: run_masked(ops, c, f) for f in MASKED_FORMS}
        for f in MASKED_FORMS:
            check_masked(c, outs[f], _F(backend, "masked_prob"))
        assert bits_equal(outs["inplace"]["dlogits"], outs["both"]["dlogits"]) and bits_equal(outs["inplace"]["sums"], outs["both"]["sums"])
    for c in PAIR_CASES:
        check_pair(c, run_pair(ops, c), _F(backend, "pairwise_reg"))
    for c in ADV_CASES:
        check_adv(c, run_adv(ops, c), _F(backend, "adv_head"))
    for c in ONEHOT_CASES:
        check_onehot(c, run_onehot(ops, c))


# ---- planted faults -------------------------------------------------------------------------------------------------------------------------
def _rejected(fn, match=None):
    with pytest.raises(AssertionError, match=match):
        fn()


def test_planted_faults_in_the_vocab_kernels_are_rejected():
    c, c346 = V342, VOCAB_BY_ID["B7-T23-E342-ld346-all-randn3"]
    _rejected(lambda: check_vocab(c, run_vocab(StepOps("drop_tail_column"), c)), "x max")          # column 341, a lane's sixth entry, left out of the sum
    _rejected(lambda: check_vocab(c, run_vocab(StepOps("logp_tb"), c)), "logp")                    # logp_bt written at [t][b]
    _rejected(lambda: check_vocab(c, run_vocab(StepOps("target_tb"), c)), "x max")                 # target read at [t][b]
    _rejected(lambda: check_vocab(c346, run_vocab(StepOps("pad_write"), c346)), "padding column")
    _rejected(lambda: check_vocab(c, run_vocab(StepOps("nan"), c)), "dlogits")
    _rejected(lambda: check_vocab_bwd(c346, run_vocab_bwd(StepOps("pad_write"), c346)), "padding column")
    _rejected(lambda: check_vocab_bwd(c, run_vocab_bwd(StepOps("nan"), c)), "dlogits")
    # a swap of the two index mappings is invisible when B == 1: the table needs B != T, both above 1
    c15 = VOCAB_BY_ID["B1-T5-E342-ld344-all-randn3"]
    check_vocab(c15, run_vocab(StepOps("logp_tb"), c15)), check_vocab(c15, run_vocab(StepOps("target_tb"), c15))
    # a -inf logit whose gradient is not exactly zero, and a -inf missing from logp
    cn = VOCAB_BY_ID["B7-T23-E342-ld344-all-ninf"]
    bufs = run_vocab(StepOps(), cn)
    r, col = 4, int(torch.nonzero(torch.isneginf(vocab_inputs(cn)["x"][4]))[0])
    bufs["dlogits"][r, col] = 1e-30
    _rejected(lambda: check_vocab(cn, bufs), "exactly zero")
    bufs = run_vocab(StepOps(), cn)
    b, t = r % 7, r // 7
    bufs["logp"].view(-1, 342)[b * 23 + t, col] = -1e30
    _rejected(lambda: check_vocab(cn, bufs), "-inf expected")
    # grad_scale = 0 and E = 1: exactly zero, not small
    for cid in ("B7-T23-E342-ld344-gs0-randn3", "B7-T23-E1-ld4-all-randn3"):
        cz = VOCAB_BY_ID[cid]
        bufs = run_vocab(StepOps(), cz)
        bufs["dlogits"][3, 0] = 1e-30
        _rejected(lambda: check_vocab(cz, bufs), "exactly zero")
    # a row past the last one written
    bufs = run_vocab(StepOps(), c)
    bufs["nll"][161] = 0.0
    _rejected(lambda: check_vocab(c, bufs), "past its last row")


def test_old_metric_accepts_a_ten_percent_error_in_a_low_probability_column():
    c = VOCAB_BY_ID["B7-T23-E342-ld344-all-lowp"]
    rec = vocab_references(c)
    bufs = run_vocab(StepOps(), c)
    check_vocab(c, bufs)
    ref = rec["ref64"]["dlogits"]
    col = 32 + int(ref[:16, 32:48].abs().amax(0).argmax())
    assert float(ref[:, col].abs().max()) < 1e-4 * f32(0.37)                       # probabilities below 1e-4
    bufs["dlogits"][:161, col] *= 1.1
    assert old_metric_accepts(bufs["dlogits"][:161, :342], ref) and old_metric_accepts(bufs["dlogits"][:161, :342], rec["fake32"]["dlogits"])
    _rejected(lambda: check_vocab(c, bufs), "x max")


def test_planted_faults_in_the_other_kernels_are_rejected():
    for c in ARGMAX_CASES:
        if c["B"] == 13 and c["E"] in (65, 342):
            _rejected(lambda: check_argmax(c, run_argmax(StepOps("last_index"), c)), "first-index argmax")
    for cid in ("Tr64-B9-C3-wave-train", "Tr65-B9-C3-loop-train"):
        c = TIME_BY_ID[cid]
        _rejected(lambda: check_time(c, run_time(StepOps("cnt_miss_last"), c)), "dlogits")
        bufs = run_time(StepOps(), c)
        bufs["nll_bc"][0, 1] = 1e-30                                               # a column without a hit
        _rejected(lambda: check_time(c, bufs), "exactly zero")
    for c in MASKED_CASES:
        if c["range_name"] in ("reference", "overlap") and c["rows"] == 5:
            _rejected(lambda: check_masked(c, run_masked(StepOps("inclusive_hi"), c, "both")), "x max")
    c = [c for c in MASKED_CASES if c["id"] == "rows5-E342-ld344-reference"][0]
    _rejected(lambda: check_masked(c, run_masked(StepOps("pad_write"), c, "both")), "padding column")
    _rejected(lambda: check_masked(c, run_masked(StepOps("nan"), c, "grad")), "dlogits")
    for c in PAIR_CASES:
        if c["tiny"]:
            _rejected(lambda: check_pair(c, run_pair(StepOps("sign_f32"), c)), "loss_rows")
    for c in ADV_CASES:
        if c["B"] >= 5 and c["variant"] in ("full", "nogz"):
            _rejected(lambda: check_adv(c, run_adv(StepOps("gate_ge"), c)), "pre == 0|exactly zero")           # the planted pre == 0 row opens
        if c["variant"] in ("full", "noda"):
            _rejected(lambda: check_adv(c, run_adv(StepOps("gz_add"), c)), "g_z")
    c = [c for c in ADV_CASES if c["id"] == "B9-Z65-ldz72-full"][0]
    bufs = run_adv(StepOps(), c)
    bufs["g_z"][0, 65] = 0.0
    _rejected(lambda: check_adv(c, bufs), "column >= Z")
    for c in ONEHOT_CASES:
        if c["rows"] >= 5 and c["V"] > 1:
            _rejected(lambda: check_onehot(c, run_onehot(StepOps("last_index"), c)), "first-index argmax")
    # a NaN in any quantity fails whatever the restatement's error is
    c = TIME_BY_ID["Tr70-B5-C5-loop-train"]
    bufs = run_time(StepOps(), c)
    bufs["logp"][17] = float("nan")
    _rejected(lambda: check_time(c, bufs), "logp")
    rec = vocab_references(V342)
    got = {k: v.clone() for k, v in rec["fake32"].items()}
    assert check_quantities(rec, got, SCAN_F_CAP)[0] <= 1.0
    got["nll"][5, 0] = float("inf")
    _rejected(lambda: check_quantities(rec, got, SCAN_F_CAP), "nll")
