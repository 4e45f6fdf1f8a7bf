"""CPU self-test of tests/helpers_latent.py, the case table, float64 references and checkers that tests/test_gpu_latent.py applies to fn_latent_fwd and
fn_latent_bwd of csrc/loss.hip.  tests/fake_ops.FakeOps (float32 autograd of the documented loss) and helpers_latent.LatentStepOps (the documented
formulas in float32) stand in for the kernels, through the same drivers.

It shows that the table has the properties its ids claim, that the input conditions hold for every case, that the backward formula on the unrounded
float64 z / qy is autograd of the documented loss - and that on the float32-rounded qy of the init case it is not, by more than the bound could absorb,
which is why the backward reference takes qy as an input -, that every checker accepts the restatement on every case and FakeOps on the live ones, that
every planted fault - an edit of the restatement - is rejected at the final F, and that the check test_gpu_parity.py has today accepts two of them."""
import numpy as np
import pytest
import torch

from fake_ops import FakeOps
from helpers import SCAN_EPS, SCAN_F_CAP, SCAN_MIN_REF
from helpers_head import tile_errors
from helpers_latent import (BAD_SHAPES, BWD_BY_ID, BWD_CASES, BWD_FORMS, BWD_REQUIRED, BWD_W3, CAP_F, CHAIN_CASES, EVERY_FORM_SHAPES, EXACT_CASES, F32, F64,
                            FAMILIES, FWD_BY_ID, FWD_CASES, FWD_REQUIRED, LATENT_F, LATENT_REFUSALS, LIVE_GAP, LIVE_QMAX, LIVE_QMIN, LIVE_SHAPES, SAT_SECOND,
                            SHAPE_BY_ID, SHAPES, UPS, LatentStepOps, _draw, bwd_exact0, bwd_given, bwd_references, chain, check_bwd, check_fwd, f32,
                            fwd_references, latent_bwd_math, latent_condition, latent_core, latent_fwd_math, latent_inputs, latent_terms, old_check_accepts,
                            old_check_inputs, run_bwd, run_exact, run_fwd)

LIVE8 = "B21-Z65-K8-live-c-2"


def _rejected(fn, match=None):
    with pytest.raises(AssertionError, match=match):
        fn()


# ---- the case table -------------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_lane_tail_row_tail_and_component_count():
    assert {c["Z"] for c in SHAPES} == {1, 5, 63, 64, 65, 128, 200} and {c["K"] for c in SHAPES} == {1, 2, 3, 8} and {c["B"] for c in SHAPES} == {1, 3, 4, 21}
    assert [B % 4 for B in (1, 3, 4, 21)] == [1, 3, 0, 1] and 21 == 16 + 5                        # a ragged second 16-row tile
    per_lane = lambda Z: [len(range(lane, Z, 64)) for lane in range(64)]                         # noqa: E731
    assert per_lane(1) == [1] + [0] * 63 and per_lane(5).count(0) == 59 and per_lane(63) == [1] * 63 + [0]          # empty lanes
    assert per_lane(64) == [1] * 64 and per_lane(65) == [2] + [1] * 63 and per_lane(128) == [2] * 64 and per_lane(200) == [4] * 8 + [3] * 56
    assert {c["c"] for c in LIVE_SHAPES} == {0, -1, -2} and {c["Z"] for c in LIVE_SHAPES} == {1, 5, 63, 64, 65, 128, 200}
    assert {c["K"] for c in LIVE_SHAPES} == {2, 3, 8} and {c["B"] for c in LIVE_SHAPES} == {1, 3, 4, 21}
    assert {c["kind"] for c in SHAPES} == {"live", "k1", "twin", "saturated", "init"}
    assert len(FWD_CASES) == 2 * len(SHAPES) and all(FWD_BY_ID[s["id"] + "-unsup"]["sup"] is False and FWD_BY_ID[s["id"] + "-labels"]["sup"] is True for s in SHAPES)
    for s in SHAPES:
        lab, inp = latent_inputs(s)["labels"], latent_inputs(s)
        assert lab.dtype == torch.int32 and int(lab.min()) >= 0 and int(lab.max()) < s["K"] and int(lab[0]) == s["K"] - 1 and (s["B"] == 1 or int(lab[1]) == 0)
        if s["twin"] is not None:
            k0, k1 = s["twin"]
            assert k0 < k1 and torch.equal(inp["mu_lk"][k0], inp["mu_lk"][k1]) and torch.equal(inp["lv_lk"][k0], inp["lv_lk"][k1])
    # backward: every form on three shapes, unsupervised and with labels; all + w3 only on every case; the chained launches
    assert set(BWD_FORMS) == set(UPS) | {"all", "w3only", "now3", "nodmu", "null", "k1w0"}
    for sid in EVERY_FORM_SHAPES:
        for v in ("-unsup", "-labels"):
            assert {c["form"] for c in BWD_CASES if c["fwd"] == sid + v} == set(BWD_FORMS) - {"k1w0"}
    assert {SHAPE_BY_ID[s]["kind"] for s in EVERY_FORM_SHAPES} == {"live", "init"}
    for f in FWD_CASES:
        assert {"all", "w3only"} <= {c["form"] for c in BWD_CASES if c["fwd"] == f["id"]}
    assert {c["fwd"] for c in BWD_CASES if c["form"] == "k1w0"} == {f["id"] for f in FWD_CASES if f["K"] == 1}
    assert {c["fwd"] for c in CHAIN_CASES} == set(FWD_BY_ID) and {c["form"] for c in CHAIN_CASES} == {"all", "w3only", "nodmu"}
    assert BWD_FORMS["k1w0"]["w3"][0] == 0.0 and "g_ll" not in BWD_FORMS["k1w0"]["ups"] and all(w != 0 for w in BWD_W3)
    assert set(LATENT_F) == set(FAMILIES) and all(0 < F <= SCAN_F_CAP for F in LATENT_F.values())
    assert max(c["B"] for c in SHAPES) <= 300 and len(FWD_CASES) + len(BWD_CASES) + len(CHAIN_CASES) < 300


def test_input_conditions_hold_for_every_case():
    for s in SHAPES:
        inp = latent_inputs(s)
        ok, info = latent_condition(s, inp)
        assert ok, (s["id"], info)
        assert all(not latent_condition(s, _draw(s, k))[0] for k in range(inp["draw"])), "%s: not the first draw that meets the condition" % s["id"]
        if s["kind"] in ("live", "twin"):
            assert info["qmax"] <= LIVE_QMAX and info["qmin"] >= LIVE_QMIN and info["gap"] >= LIVE_GAP, (s["id"], info)
        if s["kind"] == "twin":
            assert info["twin_on_top"] > 0                                         # rows whose maximum is the tie: y must be its first index
        if s["kind"] == "saturated":
            assert info["second"] < SAT_SECOND
            q32 = latent_fwd_math(inp["pre"], inp["eps"], inp["mu_lk"], inp["lv_lk"], None, F32)["qy"]
            assert set(q32.unique().tolist()) == {0.0, 1.0}
        if s["kind"] == "init":
            q = fwd_references(FWD_BY_ID[s["id"] + "-unsup"])["out64"]["qy"]
            second = q.sort(1)[0][:, -2]
            assert float(second.max()) > 1e-6 and int((second < 2.0 ** -150).sum()) > s["B"] // 2           # half-saturated rows among dead ones
            assert info["ent_tile_min"] >= SCAN_MIN_REF                                                     # and one of them in every 16-row tile
    # make_rec asserts: finite, declared zeros exactly zero in float64 and float32, declared tiny below 2**-100, every other tile maximum >= 2**-100
    for c in FWD_CASES:
        rec = fwd_references(c)
        assert rec["tiny"] == (("t1",) if c["kind"] == "saturated" else ())
        if c["kind"] in ("live", "k1", "saturated"):
            assert rec["decided"].all()
        if not c["sup"]:
            assert float(rec["ref64"]["t2"].abs().max()) == 0.0 and float(rec["ref64"]["t3"].abs().max()) == 0.0
    for c in BWD_CASES:
        rec = bwd_references(c)
        if c["form"] == "null" or (c["K"] == 1 and c["form"] == "g_qy"):
            assert bool(rec["exact0"]["dpre"].all()) and bool(rec["exact0"]["dmu"].all())
        if c["form"] == "k1w0":
            assert bool(rec["exact0"]["dmu"].all()) and not bool(rec["exact0"]["dpre"].any())
        if c["form"] == "all" and c["kind"] == "live":
            assert not bool(rec["exact0"]["dpre"].any()) and not bool(rec["exact0"]["dmu"].any())
    # the saturated posterior with w_cls != 0: the rows' dll vanish, the KL weight of the dead component too
    c = BWD_BY_ID["B21-Z128-K2-saturated-unsup-w3only"]
    m = bwd_exact0(c, bwd_given(c)[1])
    assert int(m["dmu"].sum()) == 21 * 128 and not bool(m["dpre"].any())


# ---- the backward formula is autograd of the documented loss - on the unrounded posterior ------------------------------------------------------
def _autograd(c, form="all"):
    """(dpre, dmu [B][K Z], z, qy) in float64: autograd of sum(g . outputs) + the fused loss of include/fadernets.h, the posterior recomputed from pre"""
    inp, B, K, Z = latent_inputs(c), c["B"], c["K"], c["Z"]
    pre = inp["pre"].double().requires_grad_(True)
    mlk = inp["mu_lk"].double().unsqueeze(0).repeat(B, 1, 1).requires_grad_(True)
    core = latent_core(pre, inp["eps"].double(), mlk, inp["lv_lk"].double())
    terms = latent_terms(core, inp["labels"] if c["sup"] else None)
    w_lat, w_cls, w_clf = (f32(w) for w in BWD_W3)
    tot = sum((inp["ups"][u].double() * core[k]).sum() for u, k in zip(UPS, ("z", "mu", "s", "ll", "q")) if u in BWD_FORMS[form]["ups"])
    tot = tot + (w_lat * terms[:, 2].sum() + w_clf * terms[:, 3].sum() if c["sup"] else w_lat * terms[:, 0].sum() + w_cls * terms[:, 1].sum())
    gp, gm = torch.autograd.grad(tot, [pre, mlk])
    return gp, gm.reshape(B, K * Z), core["z"].detach(), core["q"].detach()


def _bwd64(c, z, q, form="all"):
    inp = latent_inputs(c)
    return latent_bwd_math(inp["pre"], inp["eps"], inp["mu_lk"], inp["lv_lk"], inp["labels"] if c["sup"] else None, z, q,
                           *[inp["ups"][u] if u in BWD_FORMS[form]["ups"] else None for u in UPS], torch.tensor(BWD_W3), F64)


def test_backward_formula_is_autograd_of_the_documented_loss_on_the_unrounded_posterior():
    """observed: at most 1.6e-12 of a tile maximum over the 18 live cases"""
    worst = 0.0
    for c in FWD_CASES:
        if c["kind"] != "live":
            continue
        gp, gm, z, q = _autograd(c)
        o = _bwd64(c, z, q)
        worst = max(worst, float(tile_errors(o["dpre"], gp, tc=16)[0].max()), float(tile_errors(o["dmu"], gm, tc=16)[0].max()))
    print("\nlatent_bwd_math vs autograd in float64, live cases: worst tile error %.3e" % worst)
    assert worst <= 1e-10


def test_on_a_float32_qy_the_formula_is_not_the_gradient_of_the_recomputed_posterior():
    """why the backward reference takes qy as an input: on the init case (half-saturated rows, KL means of about 1e3) the float64 formula on the
    float32-rounded z / qy differs from autograd, which recomputes the posterior from pre, by more than SCAN_F_CAP x 2**-23 of a tile maximum.
    observed: 9.9e-6 of the tile maximum of dpre, 5.2 x the cap"""
    c = FWD_BY_ID["B21-Z128-K2-init-unsup"]
    gp, gm, z, q = _autograd(c)
    exact = _bwd64(c, z, q)
    assert float(tile_errors(exact["dpre"], gp, tc=16)[0].max()) <= 1e-8             # float64's own share of that cancellation: 3.0e-10 observed
    o = _bwd64(c, z.float(), q.float())
    diff = float(tile_errors(o["dpre"], gp, tc=16)[0].max())
    print("\nlatent_bwd_math on the float32 z / qy vs autograd, init case: %.3e of a tile maximum = %.1f x SCAN_F_CAP x 2**-23" % (diff, diff / (SCAN_F_CAP * SCAN_EPS)))
    assert diff > SCAN_F_CAP * SCAN_EPS
    # and the rounding of qy, not that of z, is what does it
    only_q = float(tile_errors(_bwd64(c, z, q.float())["dpre"], gp, tc=16)[0].max())
    assert only_q > SCAN_F_CAP * SCAN_EPS


# ---- the checkers accept the stand-ins ----------------------------------------------------------------------------------------------------------
def test_checkers_accept_the_float32_restatement_on_every_case():
    ops = LatentStepOps()
    for c in FWD_CASES:
        w = check_fwd(c, run_fwd(ops, c), CAP_F)
        assert max(v[0] for v in w.values()) <= 1.0, (c["id"], w)
    for c in BWD_CASES:
        w = check_bwd(c, run_bwd(ops, c), CAP_F)
        assert max(v[0] for v in w.values()) <= 1.0, (c["id"], w)
    for c in CHAIN_CASES:
        z, q = chain(ops, c)
        w = check_bwd(c, run_bwd(ops, c, z_in=z, qy_in=q), CAP_F, z_in=z, qy_in=q)
        assert max(v[0] for v in w.values()) <= 1.0, (c["id"], w)
    for name in EXACT_CASES:
        run_exact(ops, name)


def test_checkers_accept_fakeops_on_the_live_cases():
    """FakeOps recomputes its own float32 posterior and ignores the z / qy it is handed: it is asked for on the live cases only"""
    ops, worst = FakeOps(), {}
    for c in FWD_CASES:
        if c["kind"] == "live":
            for fam, v in check_fwd(c, run_fwd(ops, c), CAP_F).items():
                worst[fam] = max(worst.get(fam, 0.0), v[0])
    for c in BWD_CASES:
        if c["kind"] == "live":
            for fam, v in check_bwd(c, run_bwd(ops, c), CAP_F).items():
                worst[fam] = max(worst.get(fam, 0.0), v[0])
    print("\nFakeOps on the live cases, worst ratio per family: %s" % ", ".join("%s %.2f" % kv for kv in sorted(worst.items())))


# ---- planted faults -------------------------------------------------------------------------------------------------------------------------
def test_planted_faults_in_the_forward_are_rejected():
    un, sup = FWD_BY_ID["B21-Z128-K2-live-c-1-unsup"], FWD_BY_ID["B21-Z128-K2-live-c-1-labels"]
    _rejected(lambda: check_fwd(un, run_fwd(LatentStepOps("kl_var"), un)), "t0")                   # KL with exp(lv) taken as the variance
    _rejected(lambda: check_fwd(sup, run_fwd(LatentStepOps("kl_var"), sup)), "t2")
    _rejected(lambda: check_fwd(un, run_fwd(LatentStepOps("ll_std"), un)), "ll|argmax")                   # likelihood with exp(lv) taken as the standard deviation
    _rejected(lambda: check_fwd(un, run_fwd(LatentStepOps("no_prior"), un)), "ll")                 # log(1/K) dropped: qy does not see it, ll does
    _rejected(lambda: check_fwd(un, run_fwd(LatentStepOps("ent_sum"), un)), "t1")                  # terms[1] as a sum over K
    _rejected(lambda: check_fwd(sup, run_fwd(LatentStepOps("clf_logq"), sup)), "t3")               # terms[3] as -log q[label]
    for sid in ("B21-Z65-K3-twin-c-1-k0=k2", "B4-Z5-K2-twin-c0-k0=k1"):
        c = FWD_BY_ID[sid + "-unsup"]
        _rejected(lambda: check_fwd(c, run_fwd(LatentStepOps("y_last"), c)), "first index")        # y as the last index on a tie
    for v in ("-unsup", "-labels"):
        c = FWD_BY_ID[LIVE8 + v]
        _rejected(lambda: check_fwd(c, run_fwd(LatentStepOps("drop_last_dim"), c)), "x max|argmax")       # dimension 64 of Z = 65, lane 0's second entry
        _rejected(lambda: check_fwd(c, run_fwd(LatentStepOps("skip_last_row"), c)), "y = -7|x max")
        _rejected(lambda: check_fwd(c, run_fwd(LatentStepOps("nan"), c)), "qy")
    # rows past the last, and the exact parts
    bufs = run_fwd(LatentStepOps(), un)
    bufs["y"][21] = 0
    _rejected(lambda: check_fwd(un, bufs), "y past its last row")
    bufs = run_fwd(LatentStepOps(), un)
    bufs["terms"][4, 3] = 1e-30
    _rejected(lambda: check_fwd(un, bufs), "exactly zero")                                         # an unsupervised launch leaves terms[:, 2:4] == 0
    c = FWD_BY_ID["B21-Z65-K1-k1-c-1-labels"]
    bufs = run_fwd(LatentStepOps(), c)
    bufs["terms"][4, 1] = -1e-30
    _rejected(lambda: check_fwd(c, bufs), "exactly zero")
    c = FWD_BY_ID["B21-Z128-K2-saturated-unsup"]
    bufs = run_fwd(LatentStepOps(), c)
    bufs["terms"][4, 1] = -1e-20
    _rejected(lambda: check_fwd(c, bufs), "below 2\\*\\*-100")
    bufs = run_fwd(LatentStepOps(), c)
    bufs["qy"][4] = 1.0 - bufs["qy"][4] * (1.0 - 2.0 ** -20)
    _rejected(lambda: check_fwd(c, bufs), "first index|exactly 1 and 0")


def test_planted_faults_in_the_backward_are_rejected():
    un, sup = BWD_BY_ID[LIVE8 + "-unsup-all"], BWD_BY_ID[LIVE8 + "-labels-all"]
    unw, supw = BWD_BY_ID[LIVE8 + "-unsup-w3only"], BWD_BY_ID[LIVE8 + "-labels-w3only"]
    for c in (un, sup, unw, supw):
        _rejected(lambda: check_bwd(c, run_bwd(LatentStepOps("no_dot"), c)), "x max")              # the softmax Jacobian without - sum_j q_j dq_j
        _rejected(lambda: check_bwd(c, run_bwd(LatentStepOps("no_inv_s"), c)), "dpre")             # dsigma without - 1/s
        _rejected(lambda: check_bwd(c, run_bwd(LatentStepOps("no_s_mul"), c)), "dpre")             # the second half of dpre not multiplied by s
        _rejected(lambda: check_bwd(c, run_bwd(LatentStepOps("dmu_no_kl"), c)), "dmu")             # dmu_lk_rows without its KL part
        _rejected(lambda: check_bwd(c, run_bwd(LatentStepOps("skip_last_row"), c)), "x max")
        _rejected(lambda: check_bwd(c, run_bwd(LatentStepOps("nan"), c)), "dpre")
    for c in (un, unw):
        _rejected(lambda: check_bwd(c, run_bwd(LatentStepOps("no_klk"), c)), "x max")              # dq without w_lat KLmean_k
    for c in (sup, supw):
        _rejected(lambda: check_bwd(c, run_bwd(LatentStepOps("no_indicator"), c)), "x max")        # the cross-entropy gradient without [k == label]
    # the same faults on the chained launch, whose reference takes the arrays the forward wrote
    z, q = chain(LatentStepOps(), un)
    _rejected(lambda: check_bwd(un, run_bwd(LatentStepOps("no_dot"), un, z_in=z, qy_in=q), z_in=z, qy_in=q), "x max")
    # declared zeros, rows past the last
    c = BWD_BY_ID[LIVE8 + "-unsup-g_mu"]
    bufs = run_bwd(LatentStepOps(), c)
    bufs["dpre"][2, 65 + 3] = 1e-30
    _rejected(lambda: check_bwd(c, bufs), "exactly zero")
    bufs = run_bwd(LatentStepOps(), un)
    bufs["dmu"][21, 0] = 0.0
    _rejected(lambda: check_bwd(un, bufs), "past its last row")


def test_what_the_present_check_accepts():
    """test_gpu_parity.test_latent_kernels: B = 11, Z = 128, K = 2, lv_lk = -4 + 0.01 randn, close(..., 1e-4) against FakeOps.  Its posterior is dead -
    every row's qy is (1, 0) to three digits or better - and a backward without w_lat KLmean_k in dq passes it: q_k (dq_k - sum_j q_j dq_j) is 0
    whatever dq holds.  A backward without - sum_j q_j dq_j does NOT pass it, although the issue that asked for this suite expected it to: with
    q = (1, 0) the fault turns dll_0 = 0 into dq_0 = g_qy_0 + w_lat KLmean_0, several hundred, and the whole-tensor error of dpre is 2.4e2 of the
    tensor maximum (0.42 with labels, where dq_0 is of order 1) - that fault needs no live posterior to be seen.  Both are rejected by the per-tile check (test_planted_faults_in_the_backward_are_rejected)."""
    ok, err, qy = old_check_accepts(FakeOps(), LatentStepOps())
    assert ok and float(qy.max(1)[0].min()) > 0.999
    assert old_check_inputs()["w3"].tolist() == [f32(0.3), f32(0.2), 0.0]
    ok, err, _ = old_check_accepts(FakeOps(), LatentStepOps("no_klk"))
    print("\npresent check, backward without w_lat KLmean_k: dpre %.3e, dmu_lk_rows %.3e of the tensor maximum (tolerance 1e-4)" % err)
    assert ok
    for sup in (False, True):
        ok, err, _ = old_check_accepts(FakeOps(), LatentStepOps("no_dot"), sup=sup)
        print("present check, backward without - dot (%s): dpre %.3e, dmu_lk_rows %.3e of the tensor maximum" % ("labels" if sup else "unsupervised", err[0], err[1]))
        assert not ok and max(err) > 0.1
    assert not old_check_accepts(FakeOps(), LatentStepOps("no_s_mul"))[0]


def test_refusal_table_names_every_required_pointer_and_shape():
    names = [r[0] for r in LATENT_REFUSALS]
    assert len(set(names)) == len(names) == (len(FWD_REQUIRED) + 2 + len(BAD_SHAPES)) + (len(BWD_REQUIRED) + 2 + len(BAD_SHAPES))
    assert FWD_REQUIRED == ("pre", "eps", "mu_lk", "lv_lk", "sigma", "z", "ll", "qy", "y", "terms") and BWD_REQUIRED == ("pre", "eps", "mu_lk", "lv_lk", "z", "qy", "dpre")
    import types
    p = types.SimpleNamespace(f="f", i="i")
    for name, fn, args, code in LATENT_REFUSALS:
        a = args(p)
        assert len(a) == (15 if fn == "fn_latent_fwd" else 19) and a[-1] is None and all(isinstance(v, int) for v in a[4:7])
        B, Z, K = a[4:7]
        bad_shape = B <= 0 or Z <= 0 or K <= 0 or K > 8
        req = (0, 1, 2, 3, 8, 9, 10, 11, 12, 13) if fn == "fn_latent_fwd" else (0, 1, 2, 3, 8, 9, 16)
        null = any(a[j] is None for j in req)
        assert code == (-1 if null else -2) and (null or bad_shape), name            # NULL is checked before shape
        assert a[7] in ("i", None) and (fn != "fn_latent_fwd" or a[12] in ("i", None))
        assert max(1, B) * max(1, Z) * 2 * min(9, max(1, K)) <= 4096                # inside the buffers the GPU test hands over
    assert np.float32(SCAN_MIN_REF) > 0
