"""Host-side schedule (engine / trainer / decode) checked WITHOUT a GPU: the C-ABI ops are replaced by their documented
semantics (tests/fake_ops.py) and results are compared with the golden fixtures / the oracle.  The same assertions
run against the real HIP kernels in test_gpu_parity.py."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

from fake_ops import FakeOps
from helpers import NOISE_PARAMS, batch_of, load_golden, make_model, relerr, sd_from
from mfn_import import load_package
from oracle import gmvae_oracle as orc


@pytest.fixture(scope="module")
def small():
    return load_golden("small")


def _tensors(g):
    b = batch_of(g)
    return (torch.from_numpy(b["d"]), torch.from_numpy(b["r"]), torch.from_numpy(b["n"]), torch.from_numpy(b["c"]),
            torch.from_numpy(g["eps_r"]), torch.from_numpy(g["eps_n"]))


def test_cpu_model_without_library_hook_raises(small):
    m = make_model(64, 32, sd_from(small, "w0/"))
    d, r, n, c, er, en = _tensors(small)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(d, r, n, c, eps=(er, en))


def test_state_dict_contract(small):
    m = make_model(64, 32)
    ref = sd_from(small, "w0/")
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys()) or set(sd.keys()) == set(ref.keys())
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
        assert torch.equal(sd[k], v), k          # seeded construction == the reference's seeded construction
    assert not m.logvar_r_lookup.weight.requires_grad and m.mu_r_lookup.weight.requires_grad


def test_dropin_forward_and_autograd(small):
    """model(...) returns the reference's nested tuple; the reference-style torch loss on top of it back-propagates
    through the single fused autograd node into .grad of exactly the parameters the reference gives a gradient."""
    m = make_model(64, 32, sd_from(small, "w0/"), ops=FakeOps())
    d, r, n, c, er, en = _tensors(small)
    pkg = load_package()
    res = m(pkg.convert_to_one_hot(d, 342), pkg.convert_to_one_hot(r, 3), pkg.convert_to_one_hot(n, 16), c, eps=(er, en))
    (out, r_out, n_out, z0, z1), (dis_r, dis_n), (z_r, z_n), (ll_r, ll_n), (qy_r, qy_n), (y_r, y_n) = res
    assert z0 == 0 and z1 == 0
    got = dict(out=out, r_out=r_out, n_out=n_out, mu_r=dis_r.mean, sigma_r=dis_r.stddev, mu_n=dis_n.mean, sigma_n=dis_n.stddev,
               z_r=z_r, z_n=z_n, ll_r=ll_r, ll_n=ll_n, qy_r=qy_r, qy_n=qy_n)
    for k, v in got.items():
        tol = 1e-4 if k.startswith("qy_") else 2e-5          # q(y|x) = softmax of differences of ~1e3 log-likelihoods: fp32-ill-conditioned (tests/helpers.py)
        np.testing.assert_allclose(v.detach().numpy(), small["fw_" + k], rtol=tol, atol=tol, err_msg=k)
    assert np.array_equal(y_r.numpy(), small["fw_y_r"]) and np.array_equal(y_n.numpy(), small["fw_y_n"])
    # reference-style loss in torch on OUR outputs (what trainer_gmm.py would do after `from gmm_model import *`)
    sd = {k: p for k, p in m.named_parameters()}
    ls = orc.loss_function(sd, got, d, r, n, 20000, beta=0.2)
    l_r, l_n = orc.latent_regularized_loss(z_r, z_n, small["r_density"], small["n_density"])
    loss = ls[0] + l_r + l_n
    np.testing.assert_allclose(float(loss.detach()), small["total_loss_unsup_20000"][0], rtol=1e-5)
    loss.backward()
    for k, p in m.named_parameters():
        ref = small.get("grad_unsup/" + k)
        if ref is None:
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        assert relerr(p.grad.numpy(), ref) < 3e-4 or np.abs(ref).max() < 1e-6, (k, relerr(p.grad.numpy(), ref))


@pytest.mark.parametrize("sup,chunk", [(False, 32), (True, 32), (False, 8), (False, 5), (False, 3)])
def test_fused_step_gradients(small, sup, chunk):
    """chunk = time steps per pipeline chunk of the decoder layers (T=20, Tr=8 here): the carried states / gradients
    across chunk boundaries must not change any result."""
    pkg = load_package()
    m = make_model(64, 32, sd_from(small, "w0/"), ops=FakeOps())
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    m.engine().chunk = chunk
    b = batch_of(small)
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"], b["a"] if sup else None)
    eps = (torch.from_numpy(small["eps_r"]), torch.from_numpy(small["eps_n"]))
    tup = tr.loss_and_grads(20000, batch, eps)
    tag = "sup" if sup else "unsup"
    np.testing.assert_allclose(tup[0], small["total_loss_%s_20000" % tag][0], rtol=1e-5)
    for k in tr.flat.names:
        ref = small["grad_%s/%s" % (tag, k)]
        e = relerr(tr.flat.G[k].numpy(), ref)
        assert e < 3e-4 or np.abs(ref).max() < 1e-6, (k, e)
    np.testing.assert_allclose(tr.grad_norm(), small["gradnorm_%s_20000" % tag][0], rtol=1e-4)


@pytest.mark.parametrize("fused,lean,order", [(False, False, "side"), (True, True, "before"), (True, False, "after")])
def test_fused_step_schedule_switches(small, fused, lean, order):
    """Engine.fused_head (projection + log-softmax + NLL + gradient seed as one op, logits never written), Engine.lean_dw (the
    <= 128-register weight-gradient instance) and Engine.dw_order (where the decoder-side weight-gradient GEMMs are issued) change
    which ops run and when, never what comes out: the reference's gradients either way."""
    pkg = load_package()
    m = make_model(64, 32, sd_from(small, "w0/"), ops=FakeOps())
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    m.engine().fused_head, m.engine().lean_dw, m.engine().dw_order = fused, lean, order
    b = batch_of(small)
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    eps = (torch.from_numpy(small["eps_r"]), torch.from_numpy(small["eps_n"]))
    tup = tr.loss_and_grads(20000, batch, eps)
    np.testing.assert_allclose(tup[0], small["total_loss_unsup_20000"][0], rtol=1e-5)
    for k in tr.flat.names:
        ref = small["grad_unsup/%s" % k]
        e = relerr(tr.flat.G[k].numpy(), ref)
        assert e < 3e-4 or np.abs(ref).max() < 1e-6, (k, e)


def test_three_fused_train_steps(small):
    """GMVAETrainer.train == the reference's train() (trainer_gmm.py:220) for 3 steps from step 19999."""
    pkg = load_package()
    m = make_model(64, 32, sd_from(small, "w0/"), ops=FakeOps())
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    b = batch_of(small)
    step = 19999
    for it in range(3):
        torch.manual_seed(99 + it)
        step, tup = tr.train(step, None, None, None, b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
        np.testing.assert_allclose(tup, small["train_tuples"][it], rtol=3e-4, err_msg="step %d" % it)
    sd = m.state_dict()
    for k, v in sd_from(small, "w3/").items():
        if k in NOISE_PARAMS:
            continue
        np.testing.assert_allclose(sd[k].numpy(), v.numpy(), rtol=0, atol=1e-4, err_msg=k)   # Adam step = 1e-3; near-zero gradients carry rounding noise
    torch.manual_seed(123)
    ev = tr.evaluate(step - 1, None, None, None, b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    np.testing.assert_allclose(ev, small["eval_tuple"], rtol=3e-4)


def test_greedy_decode_and_clean_output(small):
    pkg = load_package()
    m = make_model(64, 32, sd_from(small, "w0/"), ops=FakeOps())
    m.eval()
    z = torch.from_numpy(small["dec_z"])
    steps = small["dec_tokens"].shape[1]
    lp = m.global_decoder(z, steps)
    assert tuple(lp.shape) == (z.shape[0], steps, 342)
    assert np.array_equal(lp.argmax(-1).numpy(), small["dec_tokens"])
    np.testing.assert_allclose(lp[:, 0].numpy(), small["dec_logp_first"], rtol=1e-5, atol=1e-5)
    hand = load_golden("hand")
    for i in range(5):
        got = pkg.clean_output(torch.from_numpy(hand["clean_in_%d" % i]))
        assert np.array_equal(got, hand["clean_out_%d" % i])
    m.train()
    with pytest.raises(RuntimeError, match="self.sample"):       # train mode reads self.sample (gmm_model.py:142): none yet
        m.global_decoder(z, 3)


def test_encode_and_fader_sweep_shapes(small):
    pkg = load_package()
    m = make_model(64, 32, sd_from(small, "w0/"), ops=FakeOps())
    d, r, n, c, er, en = _tensors(small)
    m.eval()
    dis_r, dis_n = m.encode(pkg.convert_to_one_hot(d, 342))
    np.testing.assert_allclose(dis_r.mean.numpy(), small["fw_mu_r"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(dis_n.stddev.numpy(), small["fw_sigma_n"], rtol=2e-5, atol=2e-5)
    tok, z0 = pkg.fader_sweep(m, d, c, [0.75], steps=30, which="r", eps=(er, en))
    assert np.array_equal(tok[:, 0].numpy(), small["dec_tokens"])          # golden decode used z_r[:,0] = 0.75
    ll, qy = m.approx_qy_x(torch.from_numpy(small["fw_z_r"]), m.mu_r_lookup, m.logvar_r_lookup, 2)
    np.testing.assert_allclose(ll.numpy(), small["fw_ll_r"], rtol=1e-5)
    r_out, n_out, _, _ = m.sub_decoders(pkg.convert_to_one_hot(r, 3), torch.from_numpy(small["fw_z_r"]),
                                        pkg.convert_to_one_hot(n, 16), torch.from_numpy(small["fw_z_n"]))
    np.testing.assert_allclose(r_out.numpy(), small["fw_r_out"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(n_out.numpy(), small["fw_n_out"], rtol=2e-5, atol=2e-5)


def test_epoch_driver_vs_reference_training_phase(tmp_path):
    """two epochs (supervised + unsupervised halves, evaluation at step-1, checkpoint every epoch) print the same
    numbers as the reference's training_phase and save a reference-format checkpoint that loads back (CPU semantics backend)."""
    from helpers import check_epoch_run
    g = load_golden("epoch")
    pkg = load_package()
    m = make_model(64, 32, ops=FakeOps())
    saved = check_epoch_run(pkg, m, g, tmp_path, rtol=2e-4)
    for k, v in saved.items():
        if k not in NOISE_PARAMS:
            np.testing.assert_allclose(v.numpy(), g["wend/" + k], rtol=0, atol=5e-4, err_msg=k)   # 8 Adam steps of 1e-3
    # checkpoint interop (trainer_gmm.py:46-48): the file loads into a fresh model, strictly
    m2 = make_model(64, 32, ops=FakeOps(), seed=5)
    m2.load_state_dict(saved, strict=True)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, saved[k]), k


def test_vae_sibling_vs_reference():
    """model_v2.MusicAttrRegVAE + trainer.py (incl. its frozen-global-step quirk) on the same engine (CPU semantics backend)."""
    from helpers import check_vae_against_reference, make_vae_model
    pkg = load_package()
    check_vae_against_reference(pkg, make_vae_model(64, 32, ops=FakeOps()), load_golden("vae"), "cpu", rtol_fw=2e-5, tol_grad=3e-4,
                                rtol_tuple=3e-4, atol_w=1e-4)


def test_eval_side_callers_host_logic():
    """evaluators.py / eval-mode forward / fader_sweep on the CPU test backend against the reference's own evaluator and notebook
    code (tests/golden/eval.npz); the GPU suite runs the same check on the HIP kernels."""
    from helpers import check_eval_side, eval_golden
    pkg = load_package()
    m = make_model(64, 32, ops=FakeOps())
    check_eval_side(pkg, m, eval_golden("s"), "cpu")


@pytest.mark.parametrize("kind", ["single", "cvae", "fader"])
def test_siblings_host_logic(kind):
    """model_v2 single-encoder siblings + their fused trainers on the CPU test backend vs the reference's own classes / trainers"""
    from helpers import check_sibling, make_sibling, sibling_golden
    pkg = load_package()
    g = sibling_golden(kind)
    check_sibling(pkg, kind, make_sibling(kind, 64, 32, ops=FakeOps()), g, "cpu", rtol_fw=3e-5, tol_grad=3e-4, rtol_tuple=1e-4)


def test_glsr_trainer_host_logic():
    """GLSRTrainer on the CPU test backend vs the reference's trainer_glsr.py run (tests/golden/glsr.npz)"""
    from helpers import check_glsr, glsr_fixture_weights, load_golden, make_vae_model
    pkg = load_package()
    g = load_golden("glsr")
    H, Z = int(g["dims"][0]), int(g["dims"][1])
    m = make_vae_model(H, Z, ops=FakeOps())
    m.load_state_dict(glsr_fixture_weights(g, H, Z))
    check_glsr(pkg, m, g, "cpu", tol_grad=5e-4, rtol_tuple=1e-4)


def test_entry_driver_config_and_loaders():
    """train.py: the reference's JSON config (tests/golden/gmm_model_config.json = its keys and values) is read verbatim; the synthetic
    arrays go through the same dataset classes / DataLoader settings as the reference's caches; data-parallel ranks take disjoint rows."""
    import argparse
    load_package()
    from music_fader_nets_amd import train as T
    args = T.read_config(os.path.join(GOLDEN, "gmm_model_config.json"))
    assert [args[k] for k in T.CONFIG_KEYS + T.GMM_KEYS] == [128, 50, 1e-3, 0.9999, "music_attr_vae_reg_gmm_long_v", 512, 128, 0.2, 32, 2]
    # model_config_v2.json (the file trainer.py / trainer_singlevae.py / trainer_cvae.py / trainer_fader.py / trainer_glsr.py open) has no
    # num_clusters: it loads unchanged for those five, and only trainer_gmm.py's script refuses it
    v2 = os.path.join(GOLDEN, "model_config_v2.json")
    for fam in ("vae", "singlevae", "cvae", "fader", "glsr"):
        a2 = T.read_config(v2, fam)
        assert [a2[k] for k in T.CONFIG_KEYS] == [128, 30, 1e-3, 0.9999, "music_attr_vae_singlevae_8.pt", 512, 128, 0.2, 32] and "num_clusters" not in a2
    with pytest.raises(KeyError, match="num_clusters"):
        T.read_config(v2, "gmm")
    with pytest.raises(KeyError):
        import json, tempfile
        with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
            json.dump({"batch_size": 8}, f)
        T.read_config(f.name)
    opts = argparse.Namespace(data_root=None, synthetic_songs=200, seq_len=40)
    dls, sizes = T.build_loaders(args, opts, 0, 1)
    assert sizes == {"train": 160, "val": 20, "test": 20, "vgm_train": 57, "vgm_val": 3}           # 80/10/10 and 90/5/5 splits
    dls2, sizes2 = T.build_loaders(args, opts, 0, 1, "fader")
    assert sorted(dls2) == ["train", "val"] and sizes2 == {"train": 160, "val": 20, "test": 20}    # the v2 scripts read the Yamaha arrays only
    # the shuffles come from an explicit generator: the same batches whatever happened to the global generator (data-parallel ranks rely on it)
    torch.manual_seed(1)
    first = next(iter(T.build_loaders(args, opts, 0, 1, "fader", seed=7)[0]["train"]))[0]
    torch.manual_seed(2); torch.rand(5)
    again = next(iter(T.build_loaders(args, opts, 0, 1, "fader", seed=7)[0]["train"]))[0]
    assert torch.equal(first, again)
    x = next(iter(dls["train"]))
    assert [tuple(t.shape) for t in x] == [(128, 40), (128, 10), (128, 10), (128, 24), (128,), (128,)] and x[0].dtype == torch.float32
    v = next(iter(dls["vgm_train"]))
    assert len(v) == 8 and v[0].shape[0] == 32 and set(v[4].tolist()) <= {0.0, 1.0}    # arousal binarised
    assert bool((v[0] == 1).any(1).all())                                              # every song carries the inserted EOS token
    a = next(iter(T.RankShard([x], 0, 2)))
    b = next(iter(T.RankShard([x], 1, 2)))
    assert torch.equal(torch.cat([a[0], b[0]]), x[0]) and a[3].shape == (64, 24)


@pytest.mark.parametrize("family", ["vae", "singlevae", "cvae", "fader"])
def test_epoch_driver_v2_vs_reference_training_phase(family, tmp_path):
    """training_phase of the model_config_v2.json trainers (tests/golden/epoch_v2.npz: the reference's own loops, two epochs) on the CPU
    semantics backend: same lines, same checkpoint.  (GLSR: gpu suite only - four 100-step decodes per step.)"""
    from helpers import check_epoch_v2_run
    check_epoch_v2_run(load_package(), family, load_golden("epoch_v2"), tmp_path, ops=FakeOps(), rtol=2e-4, atol_w=5e-4, noise=NOISE_PARAMS)


def test_data_parallel_eps_is_the_global_draw_sliced(small):
    """GMVAETrainer.draw_eps under data parallelism: rank k keeps rows [k B, (k+1) B) of the draw for the global batch (lockstep generators)"""
    pkg = load_package()
    class Ctx:                                                  # what draw_eps reads of a DataParallelContext
        def __init__(self, rank, world): self.rank, self.world, self.want_direct = rank, world, False
        def global_batch(self, b): return b * self.world
    m = make_model(64, 32, sd_from(small, "w0/"), ops=FakeOps())
    torch.manual_seed(11)
    full = pkg.GMVAETrainer(m, dist_ctx=None).draw_eps(12, 5)
    got = []
    for rank in range(3):
        torch.manual_seed(11)
        got.append(pkg.GMVAETrainer(m, dist_ctx=Ctx(rank, 3)).draw_eps(4, 5))
    for k in range(2):
        assert torch.equal(torch.cat([g[k] for g in got]), full[k])
    assert not torch.equal(got[0][0], got[1][0])


def test_stale_weight_images_are_detected(small):
    """an unmodified reference loop updates parameters in place (optimizer.step()) and never calls weights_changed(): engine() notices the
    parameters' version counters and re-derives its transposed / fragment images"""
    m = make_model(64, 32, sd_from(small, "w0/"), ops=FakeOps())
    eng = m.engine()
    calls = []
    orig = eng.refresh_weights
    eng.refresh_weights = lambda: (calls.append(1), orig())[1]
    m.engine(); m.engine()
    assert not calls
    with torch.no_grad():
        m.grucell_g.weight_hh.mul_(1.5)
    m.engine()
    assert len(calls) == 1
    m.engine()
    assert len(calls) == 1


def test_direct_calls_have_autograd(small):
    """encode / sub_decoders / global_decoder / approx_qy_x called directly in train mode (the reference allows it, gmm_model.py:82-218): one
    autograd node each, values and gradients against torch autograd of the oracle (host schedule on the CPU test backend)"""
    from helpers import check_direct_call_autograd
    pkg = load_package()
    m = make_model(64, 32, sd_from(small, "w0/"), ops=FakeOps())
    check_direct_call_autograd(pkg, m, small, "cpu", tol=2e-4)


@pytest.mark.parametrize("kind", ["single", "cvae", "fader"])
def test_sibling_forward_has_autograd(kind):
    """single-encoder drop-ins in a reference-style loop (forward -> torch loss -> loss.backward() -> optimizer.step()): one autograd node
    behind forward (+ one behind the Fader heads), gradients = the reference's own (host schedule on the CPU test backend)"""
    from helpers import check_sibling_autograd, make_sibling, sibling_golden
    pkg = load_package()
    g = sibling_golden(kind)
    H, Z = int(g["dims"][0]), int(g["dims"][1])
    m = make_sibling(kind, H, Z, ops=FakeOps())
    check_sibling_autograd(pkg, kind, m, g, "cpu", tol_grad=2e-4)


def test_generated_k_loops_wait_counts():
    """the hand-counted `s_waitcnt vmcnt(n)` of the generated K-loop statements against the issue order of their memory operations (csrc/check_kloops.py):
    no arrival may be posted while an exchange-slab store of the statement can still be in flight, no MFMA may read a register a load is still allowed
    to be writing.  Round 5: the arrival wait of fn_rs_bwd_t1_main was one operation too lenient - a real defect, unrelated to the rare eager-step
    nondeterminism of profiles/r05_eager_nondeterminism.txt (its rate did not change with the fix).  All four headers (42 statements): the four
    fn_kloop_* statements of kloop_asm.h request their ring themselves and are walked from an empty queue - and raising any single one of their 192 ring
    waits by one is a finding.  Also: the committed headers equal a regeneration, whatever KLOOP* variables the environment holds (the generators read none)."""
    import importlib.util
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "music-fader-nets_amd", "csrc")
    spec = importlib.util.spec_from_file_location("check_kloops", os.path.join(csrc, "check_kloops.py"))
    ck = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ck)
    heads = [os.path.join(csrc, h) for h in ("kloop2_asm.h", "kloop3_asm.h", "kloop4_asm.h", "kloop_asm.h")]
    for h in heads:
        assert os.path.exists(h), "%s missing: run __graft_entry__.build()" % h
    assert ck.main(heads) == 0
    # the walk of kloop_asm.h is not vacuous: every single ring wait, one too lenient, is found
    import re
    st = ck.statements(heads[3])
    nwaits = {}
    for name in ("fn_kloop_fwd_h512_k512", "fn_kloop_fwd_h512_k256", "fn_kloop_bwd_h512_k1536", "fn_kloop_bwd_h512_k768"):
        lines = st[name]
        assert ck.walk(name, lines, []) == []
        # (the closing `s_waitcnt vmcnt(0) lgkmcnt(0)` is not a ring wait: what it covers is read by the caller, behind the statement)
        ring_waits = [i for i, l in enumerate(lines) if re.fullmatch(r"s_waitcnt vmcnt\(\d+\)", l)]
        for i in ring_waits:
            mutated = list(lines)
            mutated[i] = "s_waitcnt vmcnt(%d)" % (int(lines[i][len("s_waitcnt vmcnt("):-1]) + 1)
            assert ck.walk(name, mutated, []), "%s: wait %d (%s) raised by one is not found" % (name, i, lines[i])
        nwaits[name] = len(ring_waits)
    assert list(nwaits.values()) == [32, 16, 96, 48], nwaits
    # the headers the library was built from are what the generators produce in a clean environment
    import subprocess
    import sys
    import tempfile
    env = {k: v for k, v in os.environ.items() if not k.startswith("KLOOP")}
    with tempfile.TemporaryDirectory() as td:
        for gen, head in (("gen_kloop.py", "kloop_asm.h"), ("gen_kloop2.py", "kloop2_asm.h"), ("gen_kloop3.py", "kloop3_asm.h"), ("gen_kloop4.py", "kloop4_asm.h")):
            out = os.path.join(td, head)
            subprocess.run([sys.executable, os.path.join(csrc, gen), out], check=True, env=env, cwd=csrc)
            assert open(out).read() == open(os.path.join(csrc, head)).read(), "%s differs from a clean regeneration by %s" % (head, gen)
        # and a stray variable of the former experiment switches (or any other) cannot reach a production header
        stray = dict(env, KLOOP2_ARR0="1", KLOOP2_RING0="1", KLOOP4_NT="1")
        for gen, head in (("gen_kloop2.py", "kloop2_asm.h"), ("gen_kloop4.py", "kloop4_asm.h")):
            out = os.path.join(td, "stray_" + head)
            subprocess.run([sys.executable, os.path.join(csrc, gen), out], check=True, env=stray, cwd=csrc)
            assert open(out, "rb").read() == open(os.path.join(csrc, head), "rb").read(), "%s changes with KLOOP* variables in the environment" % head


def test_isa_wait_checker_finds_an_uncovered_asm_load(tmp_path):
    """csrc/check_isa_waits.py (run by the Makefile on the compiled kernels): a register that an asm-issued load may still be writing must not be touched
    before a vmcnt wait has covered the load - across loop back-edges too.  Synthetic instruction streams: the round-5 decode race (a fill load issued
    behind the ring loads, used after a wait that only covers the ring) is a finding, the fixed order is not; a software-pipelined ring is followed
    around its loop; a load overwriting an older pending load's destination is ordered behind it."""
    import importlib.util
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "music-fader-nets_amd", "csrc")
    spec = importlib.util.spec_from_file_location("check_isa_waits", os.path.join(csrc, "check_isa_waits.py"))
    ck = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ck)

    def run(body):
        f = tmp_path / "k.s"
        f.write_text("_Z4testv:\n" + body + "\ts_endpgm\n.Lfunc_end0:\n")
        return ck.main([str(f)], jobs=1)
    asm = lambda ins: "\t;;#ASMSTART\n\t%s\n\t;;#ASMEND\n" % ins
    ring = asm("global_load_dwordx4 v[0:3], v[40:41], off") + asm("global_load_dwordx4 v[4:7], v[40:41], off")
    fill = asm("global_load_dwordx4 v[8:11], v[42:43], off")
    # the fill load is the YOUNGEST operation: vmcnt(1) covers the two ring loads only
    assert run(ring + fill + "\ts_waitcnt vmcnt(1)\n\tv_mfma_f32_16x16x4_f32 v[20:23], v0, v4, v[20:23]\n\tds_write_b128 v30, v[8:11]\n\ts_waitcnt vmcnt(0)\n") == 1
    assert run(ring + fill + "\ts_waitcnt vmcnt(1)\n\tv_mfma_f32_16x16x4_f32 v[20:23], v0, v4, v[20:23]\n\ts_waitcnt vmcnt(0)\n\tds_write_b128 v30, v[8:11]\n") == 0
    # a two-slot ring around a loop: slot 0 is used one trip after its request, behind vmcnt(1) - correct; with vmcnt(2) the use races the load
    loop = (asm("global_load_dwordx4 v[0:3], v[40:41], off") + ".LBB0_1:\n" + asm("global_load_dwordx4 v[4:7], v[40:41], off") + "\ts_waitcnt vmcnt(%d)\n"
            "\tv_add_f32 v20, v0, v20\n" + asm("global_load_dwordx4 v[0:3], v[40:41], off") + "\ts_waitcnt vmcnt(%d)\n\tv_add_f32 v20, v4, v20\n"
            "\ts_cbranch_scc1 .LBB0_1\n\ts_waitcnt vmcnt(0)\n")
    assert run(loop % (1, 1)) == 0
    assert run(loop % (2, 1)) == 1
    # load -> load on the same destination is ordered; a VALU write of a pending destination is not
    assert run(asm("global_load_dwordx4 v[0:3], v[40:41], off") + asm("global_load_dwordx4 v[0:3], v[42:43], off") + "\ts_waitcnt vmcnt(0)\n\tv_mov_b32 v9, v0\n") == 0
    assert run(asm("global_load_dwordx4 v[0:3], v[40:41], off") + "\tv_mov_b64 v[2:3], v[8:9]\n\ts_waitcnt vmcnt(0)\n") == 1
    # the build ran it on the real kernels
    assert os.path.exists(os.path.join(csrc, "isa.checked")), "run __graft_entry__.build(): csrc/Makefile checks the compiled kernels (isa.checked)"


def test_ring_driver_schedule_under_sanitizers(tmp_path):
    """csrc/ring_core.h (the register ring of the LDS-free decode K loops) compiled for the host with recording stubs for the counted wait and the
    scheduling barrier (csrc/host/ring_check.cpp, a stand-alone program, nothing preloaded): PF in {1, 2, 4, 8}, NL in {1, 4, 7}, 0 .. 3 PF + 2 steps,
    both entry forms and the parity form, under the in-order retirement model of check_isa_waits.py - 0 findings."""
    import subprocess
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "music-fader-nets_amd", "csrc", "host", "ring_check.cpp")
    exe = str(tmp_path / "ring_check")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-Wall", "-Werror", src, "-o", exe], check=True, capture_output=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
    assert "FINDING" not in p.stdout and p.stdout.strip().endswith("648 schedules, 0 findings"), p.stdout[-2000:]


def test_gemm_plan_invariants_under_sanitizers(tmp_path):
    """csrc/gemm_plan.h (the one place that decides what fn_gemm_f32 / fn_gru_dwhh_f32 launch) compiled for the host (csrc/host/gemm_plan_check.cpp, a
    stand-alone program, nothing preloaded): over shapes, layouts, flag bits, alignments, K ranges asked for and compute-unit counts every plan's K
    ranges cover K in whole blocks of the instance's granularity, its grid covers tiles x ranges or is the walking form, a reduction exists exactly
    when K is split, and the kernels without bounds checks get whole aligned tiles only - 0 findings."""
    import subprocess
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "music-fader-nets_amd", "csrc", "host", "gemm_plan_check.cpp")
    exe = str(tmp_path / "gemm_plan_check")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-Wall", "-Werror", src, "-o", exe], check=True, capture_output=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
    assert "FINDING" not in p.stdout and p.stdout.strip().endswith("1847295 plans, 0 findings"), p.stdout[-2000:]


def test_gru_plan_invariants_under_sanitizers(tmp_path):
    """csrc/gru_plan.h (the one place that decides what fn_gru_seq_fwd / fn_gru_seq_bwd / fn_gru_cell_f32 launch) compiled for the host
    (csrc/host/gru_plan_check.cpp, a stand-alone program, nothing preloaded): the table of return codes, and over scans, shapes, variant bits, forced
    row blocks, alignments, compute units and budgets every plan's grid is groups x slices within the counters, the LDS and one workgroup per compute
    unit, the per-step candidate is last, bf16 x 6 has one candidate or none, fn_gru_*_x6_ok agree with the plan; the same for the cell - 0 findings."""
    import subprocess
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "music-fader-nets_amd", "csrc", "host", "gru_plan_check.cpp")
    exe = str(tmp_path / "gru_plan_check")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-Wall", "-Werror", src, "-o", exe], check=True, capture_output=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
    assert "FINDING" not in p.stdout and p.stdout.strip().endswith("49 return codes, 3400000 plans, 0 findings"), p.stdout[-2000:]


def test_decode_plan_invariants_under_sanitizers(tmp_path):
    """csrc/decode_plan.h (the one place that decides what fn_decode_greedy / fn_decode_forced / fn_out_argmax_f32 launch) compiled for the host
    (csrc/host/decode_plan_check.cpp, a stand-alone program, nothing preloaded): the table of return codes, a literal table of plans, and over
    B 1 .. 2049, H, V, compute units, forced or not every plan's grid is replicas x role set within one workgroup per compute unit, its blocks cover B
    within the counters, LDS fits, the four workspace regions are disjoint and end inside fn_decode_ws_bytes; the output layer's kernel by K, grid and
    LDS - 0 findings."""
    import subprocess
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "music-fader-nets_amd", "csrc", "host", "decode_plan_check.cpp")
    exe = str(tmp_path / "decode_plan_check")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-Wall", "-Werror", src, "-o", exe], check=True, capture_output=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
    assert "FINDING" not in p.stdout and p.stdout.strip().endswith("138 return codes and table entries, 1056510 plans, 0 findings"), p.stdout[-2000:]


def test_fake_ops_do_not_read_an_output_they_overwrite():
    """beta == 0 means the output is write-only, as in the kernels (gemm.hip: `if (beta != 0.f)`): the engine hands over uninitialised
    buffers, and 0 x NaN is NaN.  (FakeOps.gru_dwhh once formed beta * dW: the gradient comparison above failed whenever the allocator
    returned memory that held a NaN.)"""
    ops = FakeOps()
    torch.manual_seed(0)
    nan = lambda *s: torch.full(s, float("nan"))
    H, R = 32, 10
    dgx, dghn, hp = torch.randn(R, 3 * H), torch.randn(R, H), torch.randn(R, H)
    dW = nan(3 * H, H)
    ops.gru_dwhh(dgx, dghn, hp, dW)
    assert torch.equal(dW, torch.cat([dgx[:, :2 * H], dghn], dim=1).t() @ hp)
    ops.gru_dwhh(dgx, dghn, hp, dW, beta=1.0)
    assert torch.allclose(dW, 2 * torch.cat([dgx[:, :2 * H], dghn], dim=1).t() @ hp)
    A, B = torch.randn(R, H), torch.randn(7, H)
    Cm = nan(R, 7)
    ops.gemm(A, B, Cm)
    assert torch.equal(Cm, A @ B.t())
    Cm = nan(R, 7)
    ops.gemm_multi([dict(C=Cm, segs=[(A, B)])])
    assert torch.equal(Cm, A @ B.t())
    out = nan(H)
    ops.colsum(A, out)
    assert torch.equal(out, A.sum(0))
    out = nan(1)
    ops.sum(A, out)
    assert torch.equal(out, A.sum().view(1))
