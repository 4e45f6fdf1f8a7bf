"""Reconstruction report on a real MI355X: fn_token_score and fn_match_rows on every case the CPU tests run through the two statements and the host
twin (pred, rank and every count exact, nll inside the float64 bound of tests/helpers_report.py, nll_sum bit for bit, sentinel columns and NaN padding,
a second launch with the same bits, pred equal to fn_vocab_argmax's token), the class-argmax rows on the logp_bt of fn_time_logsoftmax, and
reconstruction_report / score_tokens / evaluation_phase end to end at hidden 64, B 5, T 20, Tr 16."""
import re

import numpy as np
import pytest
import torch

import helpers_report as hr
from helpers import make_model
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOKEN_CASES = hr.token_cases()
MATCH_CASES = hr.match_cases()
PAD = 3


def _ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(DEV)


def _sentinel(shape, dtype):
    return torch.full(shape, hr.INT_SENTINEL, dtype=dtype, device=DEV)


@pytest.mark.parametrize("case", TOKEN_CASES, ids=[c["tag"].replace(" ", "_") for c in TOKEN_CASES])
def test_token_score_kernel(case):
    """x as strided rows of a NaN-padded storage cut behind the last row's last float, a target with sentinel columns, outputs as views of
    sentinel-filled buffers; all three outputs at once, then each alone, then the first launch again"""
    ops = _ops()
    B, T, V = case["B"], case["T"], case["V"]
    ref = hr.token_score_ref(case["x"], case["target"])
    store = torch.from_numpy(case["store"][:case["n_x"]].copy()).to(DEV)
    target = _sentinel((B, T + 2), torch.int32)
    target[:, :T] = torch.from_numpy(case["target"]).to(DEV)

    def launch(want):
        bufs = dict(pred=_sentinel((B, T + PAD), torch.int32), nll=_sentinel((B, T + PAD), torch.float32), rank=_sentinel((B, T + PAD), torch.int32))
        ops.token_score(store, case["stride_b"], case["stride_t"], B, T, V, target=target[:, :T] if want != ("pred",) else None,
                        **{k: bufs[k][:, :T] for k in want})
        return {k: v.cpu().numpy() for k, v in bufs.items()}

    first, alone = launch(("pred", "nll", "rank")), {k: launch((k,)) for k in ("pred", "nll", "rank")}
    again = launch(("pred", "nll", "rank"))
    torch.cuda.synchronize()
    got = {k: v[:, :T] for k, v in first.items()}
    hr.same_exact(got, ref, ("pred", "rank"), case["tag"])
    worst = hr.check_nll(got["nll"], case["x"], case["target"], case["tag"])
    print("%s: worst nll ratio %.2f" % (case["tag"], worst))
    for k, v in first.items():
        assert (v[:, T:] == hr.INT_SENTINEL).all(), (case["tag"], k, "a column behind T was written")
        assert np.array_equal(v.view(np.int32), again[k].view(np.int32)), (case["tag"], k, "a second launch differs")
        assert np.array_equal(v.view(np.int32), alone[k][k].view(np.int32)), (case["tag"], k, "alone")
        assert all((alone[k][o] == hr.INT_SENTINEL).all() for o in first if o != k), (case["tag"], k, "an output that was not asked for was written")
    assert torch.equal(target[:, T:].cpu(), torch.full((B, 2), hr.INT_SENTINEL, dtype=torch.int32))
    # fn_vocab_argmax on the same rows
    rows = torch.from_numpy(case["x"].reshape(B * T, V)).to(DEV)
    tok = torch.empty(B * T, dtype=torch.int32, device=DEV)
    ops.vocab_argmax(rows, V, None, tok)
    assert np.array_equal(tok.cpu().numpy().reshape(B, T), got["pred"]), case["tag"]


@pytest.mark.parametrize("rows", hr.MATCH_ROWS)
def test_match_rows_kernel(rows):
    ops = _ops()
    for c in (c for c in MATCH_CASES if c["rows"] == rows):
        T, pad = c["T"], c["pad"]
        ref = hr.match_rows_ref(c["pred"], c["target"], c["trim"], c["nll"], c["rank"], c["topk"])

        def wide(a, fill):
            t = torch.full((rows, T + pad), fill, dtype=torch.from_numpy(a).dtype, device=DEV)
            t[:, :T] = torch.from_numpy(a).to(DEV)
            return t[:, :T]

        ins = dict(pred=wide(c["pred"], -77), target=wide(c["target"], 5), nll=wide(c["nll"], float("nan")), rank=wide(c["rank"], 0))

        def launch(aux):
            i32, f64 = lambda: _sentinel((rows + PAD,), torch.int32), lambda: _sentinel((rows + PAD,), torch.float64)
            out = dict(lead=i32(), len=i32(), correct=i32(), correct_topk=i32(), status=i32(), acc=f64(), nll_sum=f64())
            v = {k: t[:rows] for k, t in out.items()}
            ops.match_rows(ins["pred"], ins["target"], T, c["trim"], v["lead"], v["len"], v["correct"], v["acc"], v["status"], nll=ins["nll"] if aux else None,
                           rank=ins["rank"] if aux else None, topk=c["topk"], correct_topk=v["correct_topk"] if aux else None, nll_sum=v["nll_sum"] if aux else None)
            return {k: t.cpu().numpy() for k, t in out.items()}

        first, bare, again = launch(True), launch(False), launch(True)
        hr.same_exact({k: v[:rows] for k, v in first.items()}, ref, list(ref), c["tag"])
        hr.same_exact({k: v[:rows] for k, v in bare.items()}, ref, ("lead", "len", "correct", "acc", "status"), c["tag"] + " bare")
        assert (bare["correct_topk"] == hr.INT_SENTINEL).all() and (bare["nll_sum"] == hr.INT_SENTINEL).all()
        for k, v in first.items():
            assert (v[rows:] == hr.INT_SENTINEL).all(), (c["tag"], k, "an entry behind the last row was written")
            assert v.tobytes() == again[k].tobytes(), (c["tag"], k, "a second launch differs")


@pytest.mark.parametrize("Cc", [3, 16])
def test_class_argmax_rows(Cc):
    pkg = load_package()
    print("Cc %d: %.5f of the rows left out" % (Cc, hr.class_argmax_check(pkg, _ops(), DEV, Cc)))


def _trainer(pkg):
    m = make_model(64, 32, device=DEV)
    return m, pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)


@pytest.mark.parametrize("supervised", [False, True], ids=["unsupervised", "supervised"])
def test_reconstruction_report_end_to_end(supervised):
    """hidden 64, B 5, T 20, Tr 16: every sum is the restatement applied to the logits, logp_bt and y of the same forward, teacher-forced (fused head on
    and off) and free-running; the eight loss terms are those of GMVAETrainer.evaluate with the same noise (the fused head sums in another order)"""
    pkg = load_package()
    m, tr = _trainer(pkg)
    b = hr.report_batch()
    batch = (b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    g = torch.Generator().manual_seed(5)
    eps = tuple(torch.randn(5, 32, generator=g).to(DEV) for _ in range(2))
    labels = b["a"] if supervised else None
    ev = tr.evaluate(20000, None, None, None, *batch, is_supervised=supervised, y_label=labels, eps=eps)
    for fused in (True, False):
        m.engine().fused_head = fused
        rep = pkg.reconstruction_report(tr, batch, step=20000, eps=eps, y_label=labels, topk=5)
        assert all(v.is_cuda for v in rep["tensors"].values() if torch.is_tensor(v))
        print("worst nll ratio %.2f" % hr.check_report(rep, b, labels, True, 5))
        np.testing.assert_allclose(rep["tuple8"], ev, rtol=1e-4)
    free = pkg.reconstruction_report(tr, batch, step=20000, eps=eps, y_label=labels, teacher_forced=False)
    hr.check_report(free, b, labels, False, 5)
    zc = m.engine().buf("zc", (5, 2 * 32 + 24))
    assert torch.equal(free["tensors"]["pred_x"], pkg.greedy_decode(m, zc.clone(), 20, want_logp=False)[1])


def test_score_tokens_is_a_gather_from_the_forced_decode():
    pkg = load_package()
    m = make_model(64, 32, device=DEV)
    g = torch.Generator().manual_seed(2)
    z = torch.randn(3, 2 * 32 + 24, generator=g).to(DEV)
    tok = torch.randint(0, 342, (3, 9), generator=g)
    sc = pkg.score_tokens(m, z, tok.to(DEV))
    logp, _ = pkg.greedy_decode(m, z, 9, want_logp=True, forced=tok.to(DEV), force=9)
    x = logp.cpu().numpy()
    ref = hr.token_score_ref(x, tok.numpy())
    assert sc.logp.is_cuda and np.array_equal(sc.rank.cpu().numpy(), ref["rank"]) and sc.total.dtype == torch.float64
    hr.check_nll(-sc.logp.cpu().numpy(), x, tok.numpy(), "score_tokens")
    np.testing.assert_allclose(sc.logp.cpu().numpy(), np.take_along_axis(x, tok.numpy()[..., None], -1)[..., 0], rtol=0, atol=2e-5)
    assert [hr.stated_sum(r) for r in sc.logp.cpu().numpy()] == sc.total.cpu().tolist()


def test_evaluation_phase_prints_three_lines_per_loader():
    pkg = load_package()
    m, tr = _trainer(pkg)
    from music_fader_nets_amd.synth import synth_batch
    rs = np.random.RandomState(8)
    unsup, sup = [], []
    for B in (4, 3):
        b = synth_batch(rs, B, 12, 8)
        unsup.append((b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"]))
    b = synth_batch(rs, 3, 12, 8)
    sup.append((b["d"], b["r"], b["n"], b["c"], b["a"], b["a"], b["r_density"], b["n_density"]))
    lines = []
    torch.manual_seed(4)
    res = pkg.evaluation_phase(tr, [unsup, sup], log=lines.append, step=20000)
    num = r"(-?\d[\d.e+-]*|nan)"
    pats = [r"CE: %s  %s  %s" % (num, num, num), r"Regularized: %s  %s" % (num, num), r"Acc: %s  %s  %s  %s  %s" % ((num,) * 5)] * 2
    assert len(lines) == 6 and all(re.fullmatch(p, l) for p, l in zip(pats, lines)), lines
    assert [r["n_samples"] for r in res] == [7, 3] and all(np.isfinite(r["CE_X"]) and 0 <= r["acc_x"] <= 1 for r in res)
