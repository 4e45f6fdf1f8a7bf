"""The per-block check of the assembled training step (helpers_step.check_step_grads) on the CPU: tests/fake_ops.py stands in for the kernels under
the real Engine / trainers at every shape test_gpu_step.py runs.  Asserted here: the unmodified stand-in passes, the input condition holds, STEP_F
obeys its rule (a power of two, <= 32, at least twice the stand-in's worst ratio), and planted faults - edits of CPU arrays - are rejected, with
what the whole-tensor assertions of the suite make of each (they accept four of them; the two in dense gradients they see too)."""
import functools
import os

import numpy as np
import pytest

from fake_ops import FakeOps
from helpers_step import (GMVAE_CASES, SIBLING_CASES, STEP_F, STEP_F_CAP, block_slice, check_loss_terms, check_step_grads, gmvae_case,
                          old_metric_findings, old_sample_touches, run_c0_case, run_gmvae_case, run_sibling_case, sibling_case, step_line)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [("gmvae", c["id"], s) for c in GMVAE_CASES for s in c["steps"]] + [("sibling", c["id"], s) for c in SIBLING_CASES for s in c["steps"]]
ALL += [("fixture", "c0", 20000)]           # the hidden-512 fixture whose GPU tests (test_gpu_parity.py, c0 branches) call the checker too


@functools.lru_cache(maxsize=None)
def _run(family, cid, step, ops_cls=FakeOps):
    """(gradients, loss tuple, references) of the stand-in on one case; run once per module"""
    if family == "gmvae":
        got, tup, ref, _ = run_gmvae_case(gmvae_case(cid), step, ops=ops_cls())
    elif family == "fixture":
        got, tup, ref, _ = run_c0_case(ops_cls(), chunk=24)
    else:
        got, tup, ref, _ = run_sibling_case(sibling_case(cid), step, ops=ops_cls())
    return got, tup, ref


def _rejected(got, ref):
    """the checker's complaint about `got`, or None"""
    try:
        check_step_grads(got, ref)
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("family,cid,step", ALL, ids=["%s-%s-%d" % a for a in ALL])
def test_stand_in_passes_per_block(family, cid, step):
    got, tup, ref = _run(family, cid, step)
    st = check_step_grads(got, ref)               # asserts ratio <= STEP_F, exact zeros, the noise-only tensors (references: the input condition)
    check_loss_terms(tup, ref)
    assert 0.0 <= st["floor_share"] < 0.05         # the denominator is the stand-in's own error almost everywhere, not the 2**-24 floor
    print()
    print(step_line("%s-%s step %d" % (family, cid, step), "f32", "fake-cpu", st))


def test_F_obeys_its_rule():
    """one power of two for the whole file, <= 32, at least twice the worst ratio of the stand-in over the inputs of every GPU case; some case has
    >= 100 exactly-zero blocks and >= 300 absent tokens (so that both zero checks bite)"""
    stats = {a: check_step_grads(_run(*a)[0], _run(*a)[2]) for a in ALL}
    worst = max(st["worst"][0] for st in stats.values())
    assert STEP_F <= STEP_F_CAP == 32 and STEP_F & (STEP_F - 1) == 0
    assert worst <= STEP_F / 2, (worst, max(stats, key=lambda a: stats[a]["worst"][0]))
    assert any(st["zero_blocks"] >= 100 and st["absent_tokens"] >= 300 for st in stats.values())


def test_profile_names_F_and_every_case():
    text = open(os.path.join(ROOT, "profiles", "step_fp64_errors.txt")).read()
    assert "F = %d" % STEP_F in text.splitlines()[0]
    for family, cid, step in ALL:
        assert "%s-%s step %d" % (family, cid, step) in text, (family, cid, step)


# ---- planted faults: the new check rejects them; what the old whole-tensor metrics make of them ---------------------------------------------------------
def _case_a():
    got, _, ref = _run("gmvae", "a", 20000)
    assert _rejected(got, ref) is None and old_metric_findings(got, ref) == []
    return {k: v.copy() for k, v in got.items()}, ref


def test_fault_lowest_block_zeroed():
    got, ref = _case_a()
    k = "gru_r.weight_ih_l0"
    m = ref["m"][k]
    bi, bj = (int(x) for x in np.unravel_index(int(np.argmin(np.where(m > 0, m, np.inf))), m.shape))
    assert 0 < m[bi, bj] < 1e-3 * m.max()
    got[k][block_slice(got[k].shape, bi, bj)] = 0.0
    assert old_metric_findings(got, ref) == []
    assert "%s: block (%d, %d)" % (k, bi, bj) in (_rejected(got, ref) or "")


def _neighbour_fault(got, ref, k):
    """the quietest pair of column neighbours of gradient k: the left block overwritten with the right one's values -> (bi, bj)"""
    m = ref["m"][k]
    full = got[k].shape[1] // 32                     # whole blocks only (a ragged edge block has another shape than its neighbour)
    pair = np.maximum(m[:, :full - 1], m[:, 1:full])
    bi, bj = (int(x) for x in np.unravel_index(int(np.argmin(np.where(pair > 0, pair, np.inf))), pair.shape))
    got[k][block_slice(got[k].shape, bi, bj)] = got[k][block_slice(got[k].shape, bi, bj + 1)]
    return bi, bj


def test_fault_block_replaced_by_its_neighbour():
    """grucell_g_2.weight_hh is a dense gradient: its block maxima stay above 1.4e-2 of the tensor's maximum at every shape of this file and the stride-97
    sample touches every one of its blocks, so the whole-tensor metrics DO see a neighbour's values there (recorded, as for the dropped chunk).  Where
    a tensor has quiet blocks - gru_r.weight_ih_l0, case d: a pair at 1e-4 of the maximum - they accept the same fault; the per-block check rejects both."""
    got, ref = _case_a()
    k = "grucell_g_2.weight_hh"
    bi, bj = _neighbour_fault(got, ref, k)
    assert "%s: block (%d, %d)" % (k, bi, bj) in (_rejected(got, ref) or "")
    old = old_metric_findings(got, ref)
    print("\nneighbour's values in %s block (%d, %d): the whole-tensor metrics %s" % (k, bi, bj, "reject it: %s" % old if old else "accept it"))
    assert all(name == k for name, _ in old)
    got, _, ref = _run("gmvae", "d", 20000)
    got = {n: v.copy() for n, v in got.items()}
    k = "gru_r.weight_ih_l0"
    bi, bj = _neighbour_fault(got, ref, k)
    assert old_metric_findings(got, ref) == []
    assert "%s: block (%d, %d)" % (k, bi, bj) in (_rejected(got, ref) or "")


def test_fault_one_element_off_by_a_thousandth_of_its_block():
    """in a block that neither the stride-97 sample nor the first 2 + last 2 rows touch"""
    got, ref = _case_a()
    free = [(ref["den"][k][bi, bj] / ref["m"][k][bi, bj], k, bi, bj) for k, g in ref["g64"].items() if g.ndim == 2
            for bi in range(ref["m"][k].shape[0]) for bj in range(ref["m"][k].shape[1])
            if ref["m"][k][bi, bj] > 0 and not old_sample_touches(g.shape, bi, bj)]
    assert free, "no block is free of the old samples"
    _, k, bi, bj = min(free)
    blk = got[k][block_slice(got[k].shape, bi, bj)]          # a view
    blk[blk.shape[0] // 2, blk.shape[1] // 2] += 1e-3 * ref["m"][k][bi, bj]
    assert old_metric_findings(got, ref) == []
    assert "%s: block (%d, %d)" % (k, bi, bj) in (_rejected(got, ref) or "")


def test_fault_absent_token_column_not_zero():
    got, ref = _case_a()
    k, v = "gru_n.weight_ih_l0_reverse", int(ref["absent"][len(ref["absent"]) // 2])
    assert (got[k][:, v] == 0).all()
    got[k][:, v] = 1e-9
    assert old_metric_findings(got, ref) == []
    msg = _rejected(got, ref) or ""
    assert "%s: column of token %d" % (k, v) in msg


class _LastChunkDropped(FakeOps):
    """the stand-in with the gate gradients of decoder layer 1's LAST pipeline chunk (the first backward launch of that layer) zeroed once the chunk
    has handed its state gradient on: what a dropped chunk contribution leaves in the weight gradients"""

    def gru_seq_bwd(self, scans, **kw):
        keep = [(s, s["dgx_rowsum"].clone()) for s in scans if s.get("tag") == "dec_l1" and s.get("dh_last") is None]
        super().gru_seq_bwd(scans, **kw)
        for s, rowsum in keep:
            s["dgx_all"].zero_(), s["dghn_all"].zero_()
            s["dgx_rowsum"].copy_(rowsum)


def test_fault_last_chunk_contribution_dropped():
    got, ref = _case_a()
    dropped = _run("gmvae", "a", 20000, _LastChunkDropped)[0]
    k = "grucell_g.weight_ih"
    assert not np.array_equal(dropped[k], got[k])
    got[k] = dropped[k].copy()
    assert "%s: block" % k in (_rejected(got, ref) or "")
    # the old metrics: recorded, not required (at these shapes one chunk of four carries enough of the tensor's maximum for them to see it)
    old = old_metric_findings(got, ref)
    print("\nlast chunk dropped from %s: the whole-tensor metrics %s" % (k, "reject it: %s" % old if old else "accept it"))
    assert all(name == k for name, _ in old)


# ---- the register claim of the register-stationary backward scan (first item) -----------------------------------------------------------
def _device_code_objects(path):
    """the AMDGPU code objects embedded in a HIP shared library (its offload bundles hold them as plain ELF images)"""
    import re
    import struct
    blob = open(path, "rb").read()
    for hit in re.finditer(b"\x7fELF\x02\x01", blob):
        o = hit.start()
        if struct.unpack_from("<H", blob, o + 18)[0] != 224:           # e_machine: EM_AMDGPU
            continue
        shoff, = struct.unpack_from("<Q", blob, o + 0x28)
        shentsize, shnum = struct.unpack_from("<HH", blob, o + 0x3A)
        yield blob[o:o + shoff + shentsize * shnum]


def test_bwd_rs_kernel_claims_the_whole_register_file(tmp_path):
    """gru_bwd_rs_kernel<1> / <2> must occupy all 512 registers of a SIMD lane (`asm volatile("" ::: "v255", "a255")`, gru_persist.hip): no other
    wavefront then shares a SIMD with a scan wavefront, which is all that stands between training and the unexplained corruption of a 16 x 32
    gradient patch.  Read from the kernel metadata of the library the suite loads (llvm-readelf --notes; numbers only, no instructions).
    On gfx950 the register file is unified and `.vgpr_count` is the TOTAL, accumulation registers included (gru_bwd_x6_kernel reports
    .vgpr_count 508 with .agpr_count 252: a sum of 760 exists on no SIMD), so architectural = .vgpr_count - .agpr_count and the claim
    "architectural + accumulation = 512" reads .vgpr_count == 512, with 256 of them accumulation registers (a255) and 256 architectural (v255).
    This build: .vgpr_count 512, .agpr_count 256 for both instances."""
    import shutil
    import subprocess
    from mfn_import import load_package
    load_package()
    from music_fader_nets_amd import _lib
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    root = os.path.dirname(os.path.dirname(hipcc))
    tool = next((t for t in (os.path.join(root, "llvm", "bin", "llvm-readelf"), os.path.join(root, "lib", "llvm", "bin", "llvm-readelf"),
                             "/opt/rocm/llvm/bin/llvm-readelf") if os.path.exists(t)), None) or shutil.which("llvm-readelf")
    if tool is None:
        pytest.skip("no llvm-readelf beside the hipcc that built the library")
    import re
    found = {}
    for i, image in enumerate(_device_code_objects(_lib.LIB_PATH)):
        if b"gru_bwd_rs_kernel" not in image:
            continue
        co = tmp_path / ("co%d.elf" % i)
        co.write_bytes(image)
        notes = subprocess.run([tool, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        for entry in notes.split("- .agpr_count:")[1:]:                # one metadata entry per kernel; .agpr_count is its first key
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            which = re.search(r"gru_bwd_rs_kernelILi(\d)E", name)
            if which:
                found[int(which.group(1))] = (int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)), int(entry.split()[0]))
    assert sorted(found) == [1, 2], found
    for inst, (vgpr_total, agpr) in found.items():
        arch = vgpr_total - agpr
        assert arch + agpr == 512 and agpr == 256, "gru_bwd_rs_kernel<%d>: .vgpr_count %d, .agpr_count %d" % (inst, vgpr_total, agpr)


# ---- fn_latent_bwd's softmax backward on the float32 qy: the allowance is needed, and it suffices ----------------------------------------------------
class _KernelSoftmaxBackward(FakeOps):
    """the stand-in plus the term latent_bwd_kernel's q_k (dq_k - sum_j q_j dq_j) adds on the float32 qy it is handed: rho c q_k in dll_k, rho = 1 - sum q,
    c = the dq of the largest q (helpers_step.latent_leak_allowance has the derivation); unsupervised step, no upstream g_qy"""

    def latent_bwd(self, pre, eps, mu_lk, lv_lk, labels, z, qy, g_z, g_mu, g_sigma, g_ll, g_qy, w3, dpre, dmu_lk_rows):
        super().latent_bwd(pre, eps, mu_lk, lv_lk, labels, z, qy, g_z, g_mu, g_sigma, g_ll, g_qy, w3, dpre, dmu_lk_rows)
        assert labels is None and g_qy is None and w3 is not None
        import torch
        (B, Z), K = eps.shape, mu_lk.shape[0]
        mu, s, q = pre[:, :Z].double(), torch.exp(pre[:, Z:]).double(), qy.double()
        sp = torch.exp(lv_lk.double())
        vr = (s.unsqueeze(1) / sp) ** 2
        klm = (0.5 * (vr + ((mu.unsqueeze(1) - mu_lk.double()) / sp) ** 2 - 1 - torch.log(vr))).mean(-1)
        dq = float(w3[0]) * klm + float(w3[1]) * (torch.log(q.clamp_min(1e-300)) + 1.0) / K
        lead = ((1.0 - q.sum(1)) * dq.gather(1, q.argmax(1, keepdim=True)).view(-1)).unsqueeze(1) * q            # [B][K]
        t = (z.double().unsqueeze(1) - mu_lk.double()) * torch.exp(-lv_lk.double())                              # [B][K][Z]
        ddz = -(lead.unsqueeze(-1) * t).sum(1)
        dpre[:, :Z] += ddz.float()
        dpre[:, Z:] += (ddz * eps.double() * s).float()
        dmu_lk_rows += (lead.unsqueeze(-1) * t).reshape(B, K * Z).float()


def test_latent_softmax_backward_needs_the_allowance_and_the_allowance_suffices():
    """case f with the kernel's softmax backward restated on the CPU: over F behind the rhythm posterior without latent_leak_allowance (on the MI355X:
    mu_r.weight 154.9 x, all 256 blocks; mu_r_lookup.weight 143.6 x; this restatement gives the same figures to three digits), within F with it; the
    allowance stays below 1e-3 of every block's maximum and is asked for by case f and the c0 fixture only"""
    got, _, ref = _run("gmvae", "f", 20000, _KernelSoftmaxBackward)
    assert [c["id"] for c in GMVAE_CASES if c["leak"]] == ["f"] and set(ref["leak"]) < set(ref["g64"])
    check_step_grads(got, ref)
    bare = {k: v for k, v in ref.items() if k != "leak"}
    msg = _rejected(got, bare) or ""
    assert "mu_r.weight: block" in msg and "256 of 256 blocks" in msg and "mu_r_lookup.weight: block" in msg
    for k, leak in ref["leak"].items():
        nz = ref["m"][k] > 0
        assert (leak[nz] <= 1e-3 * ref["m"][k][nz]).all(), k
    # a posterior-side fault far above the allowance is still seen where the allowance applies
    got = {k: v.copy() for k, v in got.items()}
    got["mu_r.weight"][block_slice(got["mu_r.weight"].shape, 3, 5)] *= 1.0 + 2e-3
    assert "mu_r.weight: block (3, 5)" in (_rejected(got, ref) or "")
