"""Data-parallel path through real RCCL on the GPU box (called directly through the C ABI, fn_comm_*), the HIP kernels underneath.

* one rank (any GPU box): the step with the collectives in place - all-reduce buckets beside the weight-stationary scans, all-gather
  of the regulariser inputs, all-reduce of the statistics - must be BIT-identical to the plain single-GPU step, captured into ONE
  hipGraph (the default) and with eager launches (FN_DP_GRAPH=0), with the control plane on gloo (default) or on torch's nccl backend;
* two ranks (skipped below 2 visible GPUs): half the batch each == the single-process step on the full batch, as the gloo test
  checks on the CPU backend;
* bench.py launches its own ranks when asked for --gpus N outside a launcher.
Every case runs in spawned processes so that the process group never leaks into the pytest process.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_parallel_gloo import HERE, ROOT, _free_port


def _rccl_worker(rank, world, port, out_dir, dp_graph="1", backend=None):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      FN_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0", FN_DP_GRAPH=dp_graph)
    from helpers import batch_of, load_golden, make_model, sd_from
    from mfn_import import load_package
    pkg = load_package()
    from music_fader_nets_amd import parallel
    ctx, local = parallel.init_from_env(backend)
    assert ctx is not None and ctx.world == world
    dev = "cuda:%d" % local
    gold = load_golden("small")
    b = batch_of(gold)
    B = b["d"].shape[0]
    lo, hi = rank * B // world, (rank + 1) * B // world
    m = make_model(64, 32, sd_from(gold, "w0/"), device=dev)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2, dist_ctx=ctx)
    tuples, step = [], 19999
    for it in range(4):                                       # eager, capture, replay, replay
        torch.manual_seed(99 + it)
        eps_r, eps_n = torch.randn(B, 32), torch.randn(B, 32)
        step, tup = tr.train(step, None, None, None, b["d"][lo:hi], b["r"][lo:hi], b["n"][lo:hi], b["c"][lo:hi],
                             b["r_density"][lo:hi], b["n_density"][lo:hi], eps=(eps_r[lo:hi].contiguous().to(dev), eps_n[lo:hi].contiguous().to(dev)))
        tuples.append(tup)
    torch.save(dict(tuples=tuples, flat=tr.flat.param.cpu(), gn=tr.grad_norm(), graphs=len(tr._graphs), use_graph=tr.use_graph,
                    direct=ctx.rccl is not None), os.path.join(out_dir, "r%d.pt" % rank))
    if ctx.rccl is not None:
        ctx.rccl.close()
    assert not m.engine().ops.gru_sync_error()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def _single_process_run(steps, dev="cuda:0"):
    sys.path.insert(0, HERE)
    from helpers import batch_of, load_golden, make_model, sd_from
    from mfn_import import load_package
    pkg = load_package()
    gold = load_golden("small")
    b = batch_of(gold)
    m = make_model(64, 32, sd_from(gold, "w0/"), device=dev)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    tuples, step = [], 19999
    for it in range(steps):
        torch.manual_seed(99 + it)
        step, tup = tr.train(step, None, None, None, b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
        tuples.append(tup)
    return tuples, tr.flat.param.cpu(), tr.grad_norm(), gold


@pytest.mark.gpu
@pytest.mark.parametrize("dp_graph,backend", [("1", None), ("0", None), ("1", "nccl")])
def test_single_rank_rccl_step_is_bit_identical(tmp_path, dp_graph, backend):
    mp.start_processes(_rccl_worker, args=(1, _free_port(), str(tmp_path), dp_graph, backend), nprocs=1, join=True, start_method="spawn")
    r0 = torch.load(os.path.join(tmp_path, "r0.pt"), weights_only=False)
    tuples, flat, gn, gold = _single_process_run(4)
    np.testing.assert_array_equal(np.asarray(r0["tuples"]), np.asarray(tuples))
    assert torch.equal(r0["flat"], flat)
    np.testing.assert_allclose(tuples[:3], gold["train_tuples"], rtol=5e-4)       # and both are the reference's train()
    assert r0["direct"]                                                           # the collectives went through fn_comm_* (RCCL)
    if dp_graph == "0":
        assert not r0["use_graph"] and r0["graphs"] == 0
    else:
        assert r0["use_graph"] and r0["graphs"] == 1                              # the data-parallel step IS one hipGraph


@pytest.mark.gpu
def test_two_rank_rccl_step_equals_single_process(tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 visible GPUs (the driver's multi-GPU node); the 1-GPU box runs the single-rank RCCL test")
    mp.start_processes(_rccl_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    r0 = torch.load(os.path.join(tmp_path, "r0.pt"), weights_only=False)
    r1 = torch.load(os.path.join(tmp_path, "r1.pt"), weights_only=False)
    assert torch.equal(r0["flat"], r1["flat"])
    np.testing.assert_array_equal(np.asarray(r0["tuples"]), np.asarray(r1["tuples"]))
    tuples, flat, gn, gold = _single_process_run(4)
    np.testing.assert_allclose(r0["tuples"], tuples, rtol=2e-5)
    np.testing.assert_allclose(r0["gn"], gn, rtol=1e-4)
    diff = (r0["flat"] - flat).abs()
    assert float(diff.max()) <= 4.1e-3 and float((diff > 1e-5).float().mean()) < 2e-3    # Adam noise on ~zero gradients only


def _burst_worker(rank, world, port, out_dir):
    """one rank through real RCCL, eager launches; foreign kernels (fn_occupy_cus: 8 workgroups holding 64 KB of LDS each, ~0.3 ms per burst, 9
    bursts) injected where a late collective would sit: behind the third gradient bucket.
      "joined"  = on the communicator's stream (what a lingering RCCL channel kernel is): the join in front of clip + Adam must keep them
                  away from the next step's encoder forward scan - the step just waits for them;
      "foreign" = on a third stream that only waits for the bucket (another process' kernels in the same window): they collide with
                  clip + Adam / the next step's first weight-stationary launch, whose workgroups then become resident late."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      FN_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0", FN_DP_GRAPH="0")
    import time
    from helpers import make_model
    from mfn_import import load_package
    pkg = load_package()
    from music_fader_nets_amd import parallel
    from music_fader_nets_amd.synth import synth_batch
    ctx, local = parallel.init_from_env()
    dev = "cuda:%d" % local
    B, T, Tr, NB, CYC = 256, 64, 16, 9, 600_000
    b = synth_batch(np.random.RandomState(0), B, T, Tr)
    res = {}
    for mode in ("none", "joined", "foreign", "none2"):
        m = make_model(512, 128, device=dev)
        tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2, dist_ctx=ctx)
        assert not tr.use_graph
        ops = m.engine().ops
        side = torch.cuda.Stream(device=dev)
        plain_finish = type(ctx).finish_buckets

        def finish(self, mode=mode, ops=ops, side=side):
            if mode == "joined":
                with torch.cuda.stream(self.rccl.stream):
                    for _ in range(NB):
                        ops.occupy_cus(8, 64 * 1024, CYC)
            elif mode == "foreign":
                side.wait_stream(self.rccl.stream)
                with torch.cuda.stream(side):
                    for _ in range(NB):
                        ops.occupy_cus(8, 64 * 1024, CYC)
            plain_finish(self)
        ctx.finish_buckets = finish.__get__(ctx)
        batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
        torch.manual_seed(99)
        eps = tr.draw_eps(B, T)
        step = 20000
        for _ in range(2):                                         # buffers, RCCL communicator
            tr.step_device(step, batch, eps)
            step += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(6):
            tr.step_device(step, batch, eps)
            step += 1
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 6
        assert not ops.gru_sync_error()
        res[mode] = dict(ms=dt * 1e3, flat=tr.flat.param.cpu(), tup=tr._tuple8(0.2, B, False))
        del ctx.finish_buckets
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(NB):
        ops.occupy_cus(8, 64 * 1024, CYC)
    e1.record()
    torch.cuda.synchronize()
    res["burst_ms"] = e0.elapsed_time(e1)
    torch.save(res, os.path.join(out_dir, "bursts.pt"))
    ctx.rccl.close()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.gpu
def test_bursts_behind_the_last_bucket_leave_the_step_bit_identical(tmp_path):
    """VERDICT r3 #6b: the collision window of a late collective - between the third gradient bucket and the next step's encoder forward scan
    (hidden 512, B = 256, T = 64; one rank through RCCL).  Bit-identical weights after 8 steps in every mode, sync-error word clear, and a
    bounded slow-down: bursts on the communicator's stream cost their own duration (the join holds the step back, nothing collides with a
    weight-stationary launch), bursts on a foreign stream at most twice their duration on top of that."""
    mp.start_processes(_burst_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True, start_method="spawn")
    r = torch.load(os.path.join(tmp_path, "bursts.pt"), weights_only=False)
    base = min(r["none"]["ms"], r["none2"]["ms"])
    for mode in ("joined", "foreign", "none2"):
        assert torch.equal(r[mode]["flat"], r["none"]["flat"]), mode
        assert r[mode]["tup"] == r["none"]["tup"], mode
    print("bursts %.2f ms per step: step alone %.2f ms, joined %.2f ms, foreign %.2f ms" % (r["burst_ms"], base, r["joined"]["ms"], r["foreign"]["ms"]))
    assert r["joined"]["ms"] <= base + 1.3 * r["burst_ms"] + 0.5
    assert r["foreign"]["ms"] <= base + 2.0 * r["burst_ms"] + 0.5


def _run_bench(extra, env_extra=None, timeout=900):
    env = dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
def test_bench_launches_its_own_ranks(n):
    """`python bench.py --gpus N --full` with no launcher environment prints ONE JSON line with n_gpus = N (N = 1 also runs with the
    collectives forced on, FN_FORCE_DIST=1, i.e. through RCCL)."""
    if torch.cuda.device_count() < n:
        pytest.skip("needs %d visible GPUs" % n)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    if n == 1:
        env["FN_FORCE_DIST"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "2", "--warmup", "2", "--full", "--sustain", "20", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["config"]["global_batch"] == 256 * n and out["value"] > 0
    assert 0 < out["roofline"]["frac"] < 1 and out["roofline_all"]
    assert out["roofline"]["symbol"] in out["roofline_by_symbol"] and 0 < out["roofline_scans"]["frac"] < 1
    assert out["sustained_steps"] == 20 and out["sustained_ms_per_step"] > 0
    assert out["dtype"] in ("f32", "f32/bf16x6") and out["arith"]
    assert out["comm"]["rccl_ranks"] == n and out["comm"]["rccl_rank"] == 0     # what RCCL itself reports (fn_comm_count / fn_comm_rank)
    if n == 1:
        leg = out.get("bf16x6_leg") or out.get("fp32_mfma_leg")     # the OTHER arithmetic rides beside the headline, timed in its own process
        assert leg["ms_per_step"] > 0 and abs(leg["first_step_loss"] - out["first_step_loss"]) <= 1e-4 * abs(out["first_step_loss"])
    else:
        chk = out["comm"]["dp_selfcheck"]                           # N ranks through RCCL == one process on the global batch (small shape)
        assert chk["max_rel_diff_of_the_tuples"] <= 2e-4, chk


@pytest.mark.gpu
def test_bench_plain_run_dumps_its_outputs(tmp_path):
    """A plain `python bench.py --steps 2 --warmup 2 --dump-outputs DIR` prints the headline line without anything of --full, and DIR holds
    what the last timed step computed: the loss tuple (its first entry = `last_loss`), the gradient norm and every trainable parameter,
    as float32 / float64 arrays of 64 MB at most in all."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "FN_FORCE_DIST")}
    dump = os.path.join(str(tmp_path), "out")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "2", "--dump-outputs", dump],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0 and out["higher_is_better"] is True
    assert out["unit"] == "event-tokens/s" and out["dtype"] in ("f32", "f32/bf16x6") and out["metric"]
    for k in ("roofline", "roofline_all", "sustained_ms_per_step", "first_step_loss", "cpu_baseline", "decode", "fp32_mfma_leg", "bf16x6_leg", "comm"):
        assert k not in out, k
    arrays = {f[:-4]: np.load(os.path.join(dump, f)) for f in os.listdir(dump)}
    assert arrays["loss"].shape == (8,) and arrays["grad_norm"].shape == (1,)
    assert abs(arrays["loss"][0] - out["last_loss"]) <= 1e-4 * abs(out["last_loss"])
    params = [k for k in arrays if k.startswith("params.")]
    assert params and set(arrays) == set(params) | {"loss", "grad_norm"}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20


def test_bench_respawns_under_the_launcher_without_gpus():
    """CPU container: `--gpus 2` with no WORLD_SIZE must reach the per-rank "needs an MI355X" exit through torch.distributed.run,
    not die on a WORLD_SIZE mismatch before any rank starts (round-1 behaviour)."""
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode != 0
    assert "needs an MI355X" in p.stderr and "but WORLD_SIZE" not in p.stderr, p.stderr[-2000:]
